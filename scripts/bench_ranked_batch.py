#!/usr/bin/env python3
"""Ranked batch-mode selection (dal.similarity.ranked_batch_select) beside the
plain greedy k-center selection (kcenter_select) it extends, in one process,
the two alternating.

Per shape (K13's two: 8,000,000 x 128 bf16, m = 1,024 labeled rows, k = 1,000;
and 1,000,000 x 128, m = 1,024, k = 100; uniform rows; weights = the
least-confidence batch weight of uniform T = 10 votes, so about n / 11 rows
share each of 6 values):

  ranked   host wall of ranked_batch_select (k steps, the final status read
           included; alpha = the default |C| / (|C| + m))
  plain    host wall of kcenter_select on the same pool
  ratio    ranked step over plain step.  The one derived expectation is the
           update pass's byte ratio (2 d + 21) / (2 d + 13): 1.03 at d = 128
  propose / commit   the two step entries alone for each mode, HIP events over
           repeated calls of one job; the update pass's bytes (the pool once,
           m32 read and written, 1 / ||x||, the flags, and c for the ranked
           mode) over the commit time as a fraction of the achievable HBM rate
           (6.3 TB/s)

No threshold on time.  Single device only: the sharded entry's timing is not
measured here.  One JSON line per shape on stdout; everything to --out
(default profiles/ranked_batch/bench_ranked_batch.json).

    python scripts/bench_ranked_batch.py [--rounds 3] [--shapes 5,1m] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "distributed-active-learning_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = {"5": (8_000_000, 128, 1024, 1000), "1m": (1_000_000, 128, 1024, 100), "tiny": (50_000, 128, 256, 20)}
HBM_ACHIEVABLE_BYTES_PER_S = 6.3e12  # MI355X, measured streaming rate
N_TREES = 10


def bench_shape(n, d, m, k, rounds, dev):
    import torch

    from dal import luts
    from dal import similarity as sim

    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    x = torch.rand((n, d), device=dev, dtype=torch.float32, generator=gen).to(torch.bfloat16)
    votes = torch.randint(0, N_TREES + 1, (n,), device=dev, generator=gen)
    w = torch.from_numpy(luts.batch_weight_lut("least_confidence", N_TREES)).to(dev)[votes]
    lab = torch.arange(m, device=dev, dtype=torch.int64)
    cand = torch.arange(m, n, device=dev, dtype=torch.int64)
    alpha = sim.default_alpha(n - m, m)

    def ranked():
        return sim.ranked_batch_select(x, lab, w, k, alpha=alpha, candidates=cand, device=dev)

    def plain():
        return sim.kcenter_select(x, lab, k, candidates=cand, device=dev)

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, r

    timed(ranked), timed(plain)  # warm-up: allocator, code objects
    t_ranked, t_plain = [], []
    for _ in range(rounds):  # the two alternate
        ms, sel = timed(ranked)
        t_ranked.append(ms)
        ms, _ = timed(plain)
        t_plain.append(ms)

    # the two step entries alone, HIP events over repeated calls of one job
    reps = 50

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        a.record()
        for t in range(reps):
            fn(t)
        b.record()
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b) * 1e3 / reps

    entries = {}
    for mode in ("ranked", "plain"):
        st = sim.HipKCenterSteps(dev)
        if mode == "ranked":
            st.prepare(x, 0, x[:m], cand, weights=w, alpha=alpha)
        else:
            st.prepare(x, 0, x[:m], cand)
        st.begin(reps)
        rec = st.propose(0).reshape(1, -1)
        entries[mode] = (events(lambda t: st.propose(0)), events(lambda t: st.commit(t, rec)))
        st.finish()
    bytes_plain = n * d * 2 + n * (4 + 4 + 4 + 1)
    bytes_ranked = bytes_plain + n * 8
    ranked_step = statistics.median(t_ranked) / k
    plain_step = statistics.median(t_plain) / k
    return {
        "n": n, "d": d, "m": m, "k": k, "alpha": alpha, "rounds": rounds,
        "ranked_ms": t_ranked, "plain_ms": t_plain,
        "ranked_step_ms": ranked_step, "plain_step_ms": plain_step,
        "ratio_ranked_over_plain": ranked_step / plain_step,
        "ratio_worst_round": (max(t_ranked) / k) / (min(t_plain) / k),
        "expected_update_byte_ratio": bytes_ranked / bytes_plain,
        "ranked_propose_us": entries["ranked"][0], "ranked_commit_us": entries["ranked"][1],
        "plain_propose_us": entries["plain"][0], "plain_commit_us": entries["plain"][1],
        "ranked_update_bytes": bytes_ranked, "plain_update_bytes": bytes_plain,
        "ranked_update_hbm_fraction": bytes_ranked / (entries["ranked"][1] * 1e-6) / HBM_ACHIEVABLE_BYTES_PER_S,
        "plain_update_hbm_fraction": bytes_plain / (entries["plain"][1] * 1e-6) / HBM_ACHIEVABLE_BYTES_PER_S,
        "selected_score_first_last": [float(sel.selected_scores[0]), float(sel.selected_scores[-1])],
        "selected_similarity_first_last": [float(sel.selected_similarity[0]), float(sel.selected_similarity[-1])],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="5,1m")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ranked_batch", "bench_ranked_batch.json"))
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "bench_ranked_batch needs a GPU"
    dev = torch.device("cuda:0")
    results = []
    for name in args.shapes.split(","):
        r = bench_shape(*SHAPES[name], args.rounds, dev)
        results.append(r)
        print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(dev), "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
