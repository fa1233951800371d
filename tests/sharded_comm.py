"""A TorchComm that counts the collectives a sharded operation issues, and the
spawn helper of the two-rank tests that use it."""
import os
import socket
import traceback

from dal import parallel


class _CountedDist:
    """torch.distributed with its all_reduce counted."""

    def __init__(self, dist, counts):
        self._dist, self._counts = dist, counts

    def all_reduce(self, *args, **kwargs):
        self._counts["all_reduce"] += 1
        return self._dist.all_reduce(*args, **kwargs)

    def __getattr__(self, name):
        return getattr(self._dist, name)


class CountingComm(parallel.TorchComm):
    """counts["gather"]: calls of all_gather_start / all_gather_rows from
    outside the comm (all_gather, the byte view of 16-bit rows and gloo's
    staging of device rows re-enter all_gather_start: one collective, one
    count); counts["all_reduce"]: calls through comm.dist.all_reduce."""

    def __init__(self, group=None):
        super().__init__(group)
        self.counts = {"gather": 0, "all_reduce": 0}
        self.dist = _CountedDist(self.dist, self.counts)
        self._depth = 0

    def _outermost(self, fn, t):
        self.counts["gather"] += self._depth == 0
        self._depth += 1
        try:
            return fn(t)
        finally:
            self._depth -= 1

    def all_gather_start(self, t):
        return self._outermost(super().all_gather_start, t)

    def all_gather_rows(self, row):
        return self._outermost(super().all_gather_rows, row)

    def take(self):
        """(gathers, all-reduces) since the last take."""
        got = (self.counts["gather"], self.counts["all_reduce"])
        self.counts["gather"] = self.counts["all_reduce"] = 0
        return got


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, q, run, args):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        q.put((rank, run(rank, world, *args)))
    except Exception:  # surface worker failures instead of a queue timeout
        q.put((rank, traceback.format_exc()))
        raise
    finally:
        dist.destroy_process_group()


def run_ranks(run, world, *args, timeout=240):
    """run(rank, world, *args) -> dict on ``world`` spawned gloo ranks (a
    module-level function of an importable test module); the dicts by rank."""
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_rank, args=(r, world, port, q, run, args)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=timeout) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
    for r in range(world):
        assert isinstance(res[r], dict), res[r]
    assert all(p.exitcode == 0 for p in procs)
    return [res[r] for r in range(world)]
