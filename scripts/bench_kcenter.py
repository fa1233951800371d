#!/usr/bin/env python3
"""Greedy k-center batch selection (dal.similarity.kcenter_select) beside its
composition on the earlier public surface -- k successive
diversity_select(pool, labeled + picks, 1, candidates minus picks) calls --
in one process, the two paths alternating.

Per shape (BASELINE config 5: 8,000,000 x 128 bf16, m = 1,024 labeled rows,
k = 1,000; and 1,000,000 x 128, m = 1,024, k = 100; uniform rows):

  new      host wall of kcenter_select (k steps, one status read at the end)
  comp     host wall of the composition, capped at the steps whose labeled set
           still fits the max-cosine kernel (m + t - 1 <= 4,096)
  same     the composition's picks and fp64 score bits equal the new path's
  propose  dal_kcenter_propose alone, HIP events over repeated calls
  commit   dal_kcenter_commit alone (the pick kernel + the update pass), HIP
           events; the update pass's bytes (the pool once, m32 read and
           written, 1 / ||x|| and the flags) over that time as a fraction of
           the achievable HBM rate (6.3 TB/s)

One JSON line per shape on stdout; everything to --out (default
profiles/kcenter/bench_kcenter.json).

    python scripts/bench_kcenter.py [--rounds 3] [--shapes 5,1m] [--out FILE]
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
MAX_LABELED = 4096


def bench_shape(n, d, m, k, rounds, dev):
    import torch

    from dal import similarity as sim

    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    x = torch.rand((n, d), device=dev, dtype=torch.float32, generator=gen).to(torch.bfloat16)
    lab = torch.arange(m, device=dev, dtype=torch.int64)
    cand0 = torch.arange(m, n, device=dev, dtype=torch.int64)
    steps_comp = min(k, MAX_LABELED - m + 1)

    def new():
        return sim.kcenter_select(x, lab, k, candidates=cand0, device=dev)

    def comp():
        labeled, cand, idx, sc = lab, cand0, [], []
        for _ in range(steps_comp):
            one = sim.diversity_select(x, labeled, 1, candidates=cand, device=dev)
            idx.append(one.indices)
            sc.append(one.selected_scores)
            labeled = torch.cat([labeled, one.indices])
            cand = cand[cand != one.indices]
        return torch.cat(idx), torch.cat(sc)

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, r

    timed(new), timed(comp)  # warm-up: allocator, code objects
    t_new, t_comp, same = [], [], True
    for _ in range(rounds):  # the paths alternate
        ms, sel = timed(new)
        t_new.append(ms)
        ms, (c_idx, c_sc) = timed(comp)
        t_comp.append(ms)
        same = same and bool(torch.equal(sel.indices[:steps_comp], c_idx)) and bool(
            torch.equal(sel.selected_scores[:steps_comp].view(torch.int64), c_sc.view(torch.int64)))

    # the two step entries alone, HIP events over repeated calls of one job
    reps = 50
    st = sim.HipKCenterSteps(dev)
    st.prepare(x, 0, x[:m], cand0)
    st.begin(reps)
    rec = st.propose(0).reshape(1, -1)

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        a.record()
        for t in range(reps):
            fn(t)
        b.record()
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b) * 1e3 / reps

    propose_us = events(lambda t: st.propose(0))
    commit_us = events(lambda t: st.commit(t, rec))
    st.finish()
    update_bytes = n * d * 2 + n * (4 + 4 + 4 + 1)
    new_step = statistics.median(t_new) / k
    comp_step = statistics.median(t_comp) / steps_comp
    return {
        "n": n, "d": d, "m": m, "k": k, "composition_steps": steps_comp, "rounds": rounds,
        "new_ms": t_new, "composition_ms": t_comp,
        "new_step_ms": new_step, "composition_step_ms": comp_step,
        "ratio_composition_over_new": comp_step / new_step,
        "ratio_worst_round": (min(t_comp) / steps_comp) / (max(t_new) / k),
        "same_picks": same,
        "propose_us": propose_us, "commit_us": commit_us,
        "update_bytes": update_bytes,
        "update_hbm_fraction": update_bytes / (commit_us * 1e-6) / HBM_ACHIEVABLE_BYTES_PER_S,
        "selected_score_first_last": [float(sel.selected_scores[0]), float(sel.selected_scores[-1])],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="5,1m")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kcenter", "bench_kcenter.json"))
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "bench_kcenter needs a GPU"
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
