#!/usr/bin/env python3
"""Ranked batch-mode selection step by step beside the plain k-center job: the
contenders kc_scan lists per step (the workspace's control word, copied on the
device) and each step's propose and commit times by HIP events, for the plain
job, the ranked job at its default alpha and the ranked job at alpha = 0.5.

The pool, weights and shapes are bench_ranked_batch.py's (1M x 128 for k = 100,
8M x 128 for the first 200 steps).  The event pairs and the copy sit between
the launches, so the times are above those of an undisturbed run; they compare
the modes with each other.  One line per (shape, mode) on stdout; everything to
--out (default profiles/ranked_batch/steps.json).

    python scripts/ranked_batch_steps.py [--out FILE]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "distributed-active-learning_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = {"1m": (1_000_000, 128, 1024, 100), "5": (8_000_000, 128, 1024, 200)}


def quantiles(v):
    s = sorted(v)
    return [round(s[min(int(len(s) * f), len(s) - 1)], 1) for f in (0, 0.5, 0.9, 0.99)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ranked_batch", "steps.json"))
    args = ap.parse_args()
    import torch

    from dal import luts
    from dal import similarity as sim

    assert torch.cuda.is_available(), "ranked_batch_steps needs a GPU"
    dev = torch.device("cuda:0")
    out = {}
    for name, (n, d, m, k) in SHAPES.items():
        gen = torch.Generator(device=dev)
        gen.manual_seed(0)
        x = torch.rand((n, d), device=dev, dtype=torch.float32, generator=gen).to(torch.bfloat16)
        votes = torch.randint(0, 11, (n,), device=dev, generator=gen)
        w = torch.from_numpy(luts.batch_weight_lut("least_confidence", 10)).to(dev)[votes]
        cand = torch.arange(m, n, device=dev)
        for mode in ("plain", "ranked", "ranked_half"):
            st = sim.HipKCenterSteps(dev)
            if mode == "plain":
                st.prepare(x, 0, x[:m], cand)
            else:
                st.prepare(x, 0, x[:m], cand, weights=w,
                           alpha=0.5 if mode == "ranked_half" else sim.default_alpha(n - m, m))
            st.begin(k)
            off = (-st.ws.data_ptr()) % 256  # the job's control block: fp64 threshold, fp32 mu, uint32 count
            ctl = st.ws[off:off + 16].view(torch.int32)
            counts = torch.zeros(k, dtype=torch.int32, device=dev)
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(k)]
            torch.cuda.synchronize(dev)
            for t in range(k):
                ev[t][0].record()
                rec = st.propose(t)
                ev[t][1].record()
                counts[t] = ctl[3]
                st.commit(t, rec.reshape(1, -1))
                ev[t][2].record()
            torch.cuda.synchronize(dev)
            st.finish()
            c = counts.cpu().tolist()
            pr = [ev[t][0].elapsed_time(ev[t][1]) * 1e3 for t in range(k)]
            cm = [ev[t][1].elapsed_time(ev[t][2]) * 1e3 for t in range(k)]
            out[f"{name}/{mode}"] = {"n": n, "d": d, "m": m, "steps": k, "contenders": c, "propose_us": pr,
                                     "commit_us": cm}
            print(name, mode, "min / median / p90 / p99: contenders", quantiles(c), "propose_us", quantiles(pr),
                  "commit_us", quantiles(cm), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(dev), "results": out}, f)


if __name__ == "__main__":
    main()
