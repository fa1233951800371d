#!/usr/bin/env python3
"""The warm multiclass density step: the unfused pair, the fused call
(dal_dw_step_multiclass) and the plan (dal_dw_plan_create_multiclass), same
pool, one process, the variants alternating.

Shapes: BASELINE configs 2 (100,000 x 64, T = 10), 3 (284,807 x 30, T = 100)
and 4 (2,000,000 x 256, T = 10), and config 4 with T = 100 ("4T100"); depth 4,
a forest of C = 10 classes, k = 10, every row but the first 10 unlabeled.

Device spans (HIP events; a GPU spin queued first, so that a span's launches
are all submitted before the GPU reaches its start event):

  score         dal_forest_score_multiclass_dw_blocked: the kernel without hooks
  pair          score + dal_dw_select (fast level 1): kernel, group_min_kernel, select
  fused         dal_dw_step_multiclass (DAL_STEP_WS_CLEAN): the kernel with the
                step hooks -- the group fold where dal_dw_step_multiclass_form
                says so -- and the select

  fused - pair is what the in-kernel fold costs more (or less) than the
  group_min_kernel launch it replaces; the fold is worth keeping where that is
  not positive beyond the pair's interquartile range.

Host wall of one warm engine step, the status read included (time.perf_counter
around the call, a device synchronise outside it):

  parent        the unfused route: row flags on the host side, the score entry,
                a workspace and dal_dw_select, a blocking status read
  fused         multiclass_density_step with use_graphs = False
  plan          multiclass_density_step through the cached plan
  binary_plan   density_step of a two-class forest of the same shape through its
                plan (orientation only)

Medians, interquartile ranges and every sample go to
profiles/multiclass/step_<shape>.json; without --shape every shape runs in a
fresh child process under its own time limit, and the run stops at the first
child that fails.

    python scripts/bench_multiclass_step.py [--shape 2|3|4|4T100] [--rounds 30] [--out DIR]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "distributed-active-learning_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

# shape -> (rows, features, trees, pool distribution)
SHAPES = {"2": (100_000, 64, 10, "uniform"), "3": (284_807, 30, 100, "normal"), "4": (2_000_000, 256, 10, "uniform"),
          "4T100": (2_000_000, 256, 100, "uniform")}
DEPTH, CLASSES, K, WARMUPS, CHILD_TIMEOUT_S = 4, 10, 10, 3, 420


def _stats(samples):
    q = statistics.quantiles(samples, n=4)
    return {"median": statistics.median(samples), "min": min(samples), "iqr": q[2] - q[0], "samples": samples}


def _alternate(rounds, variants, timed):
    """WARMUPS of every variant, then ``rounds`` rounds of one timed run each."""
    for _ in range(WARMUPS):
        for fn in variants.values():
            fn()
    out = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            out[name].append(timed(fn))
    return out


def run_shape(shape: str, rounds: int, out_dir: str) -> dict:
    import torch

    from dal import _lib, engine
    from dal.engine import _ptr, _stream
    from dal.forest import Forest

    lib = _lib.load()
    n, d, T, dist = SHAPES[shape]
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    x = (torch.rand if dist == "uniform" else torch.randn)((n, d), generator=gen, device=dev, dtype=torch.float32)
    state = engine.PoolState(x, excluded=range(10), device=dev)
    del x
    fm = Forest.synthetic(T, DEPTH, d, seed=1, dist=dist, n_classes=CLASSES)
    fb = Forest.synthetic(T, DEPTH, d, seed=1, dist=dist)
    unl = torch.arange(10, n, dtype=torch.int64, device=dev)
    # the caches every warm step reads
    dens, norm64, colsum = state.density_fixed(), state.norms(), state.colsum()
    derr = float(engine.density_error(state))
    xb = state.blocked_pool(fm, multiclass=True)
    if xb is None:
        raise SystemExit(f"shape {shape}: no blocked copy")
    fprep = engine._fprep(fm, state, xb)
    inner, leaf = fm.device(dev)
    lut = engine.device_multiclass_lut("entropy", T, dev)
    flags = state.row_flags(unl)[0]
    cap = engine.candidate_cap(n, K)
    form = int(lib.dal_dw_step_multiclass_form(n, d, T, DEPTH, CLASSES, K, cap, 1, 1))
    torch.cuda.synchronize(dev)

    # ---- device spans -------------------------------------------------------
    def buf(dt, *shape_):
        return torch.empty(shape_, dtype=dt, device=dev)

    counts, pred = buf(torch.uint8, n, CLASSES), buf(torch.uint8, n)
    entropy, row_index, scores = buf(torch.float64, n), buf(torch.int32, n), buf(torch.float64, n)
    keys_lo, keys_hi = buf(torch.int64, n), buf(torch.int64, n)
    out_idx, out_scores, out_keys = buf(torch.int64, K), buf(torch.float64, K), buf(torch.int64, K)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    wsb = int(lib.dal_dw_step_workspace_bytes(n, K, cap))
    ws_pair, wsp_pair = engine.workspace(wsb, dev)
    ws_step, wsp_step = engine.workspace(wsb, dev)
    ws_step.zero_()
    head = (_ptr(state.x), _ptr(xb), fprep, n, d, d, _ptr(inner), _ptr(leaf), T, DEPTH, CLASSES, _ptr(lut), _ptr(dens))
    rows = (_ptr(counts), _ptr(pred), _ptr(entropy), _ptr(row_index), _ptr(scores), _ptr(keys_lo), _ptr(keys_hi))
    outs = (_ptr(out_idx), _ptr(out_scores), _ptr(out_keys), _ptr(status), 0, _stream(dev))

    def score():
        _lib.call("dal_forest_score_multiclass_dw_blocked", *head, _lib.DAL_DENSITY_FIXED, derr, _ptr(flags), 1.0,
                  *rows, _stream(dev))

    def pair():
        score()
        _lib.call("dal_dw_select", _ptr(keys_lo), _ptr(keys_hi), _ptr(row_index), _ptr(flags), n, K, 0, _ptr(entropy),
                  1.0, _ptr(state.x), d, d, _ptr(norm64), _ptr(colsum), cap, 1, wsp_pair, wsb, *outs)

    def fused():
        _lib.call("dal_dw_step_multiclass", *head, derr, _ptr(flags), 1.0, 0, _ptr(norm64), _ptr(colsum), K, cap, 1,
                  _lib.DAL_STEP_WS_CLEAN, wsp_step, wsb, *rows, *outs)

    def span(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(600_000)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b) * 1e3

    dev_us = _alternate(rounds, {"score": score, "pair": pair, "fused": fused}, span)
    sel_pair = out_idx.cpu().tolist()
    if int(status.item()) != 0:
        raise SystemExit(f"shape {shape}: status {int(status.item())} after the device spans")

    # ---- host wall of one warm engine step ------------------------------------
    def parent():
        fl, u, n_cand = state.row_flags(unl)
        kk = min(K, n_cand)
        _, _, ent, ix, sc, klo, khi = engine.forest_score_multiclass_dw(
            state, fm, fl, dens, _lib.DAL_DENSITY_FIXED, density_err=derr, beta=1.0, want_hi=True, xb=xb)
        idx, sel, _ = engine.dw_select_local(state, fl, ix, klo, khi, ent, kk, 1.0, colsum)
        state.check_status(state.last_status)
        return idx

    def eager():
        state.use_graphs = False
        return engine.multiclass_density_step(state, unl, fm, K).indices

    def plan():
        state.use_graphs = True
        return engine.multiclass_density_step(state, unl, fm, K).indices

    def binary_plan():
        state.use_graphs = True
        return engine.density_step(state, unl, fb, K).indices

    last = {}

    def wall(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        idx = fn()
        t1 = time.perf_counter()
        torch.cuda.synchronize(dev)
        last[fn.__name__] = idx
        return (t1 - t0) * 1e6

    host_us = _alternate(rounds, {"parent": parent, "fused": eager, "plan": plan, "binary_plan": binary_plan}, wall)
    sels = {name: t.cpu().tolist() for name, t in last.items()}
    if not (sels["parent"] == sels["eager"] == sels["plan"] == sel_pair):
        raise SystemExit(f"shape {shape}: the variants' selections differ")

    D = {k: _stats(v) for k, v in dev_us.items()}
    H = {k: _stats(v) for k, v in host_us.items()}
    fold_minus_group_min = D["fused"]["median"] - D["pair"]["median"]
    plan_minus_parent = H["plan"]["median"] - H["parent"]["median"]
    res = {
        "shape": shape, "rows": n, "features": d, "trees": T, "depth": DEPTH, "classes": CLASSES, "k": K, "cap": cap,
        "form": form, "rounds": rounds, "warmups": WARMUPS, "device": torch.cuda.get_device_name(dev),
        "device_span_us": D, "host_wall_us": H,
        "fused_minus_pair_us": fold_minus_group_min,
        "fold_verdict": ("not slower than the group_min launch" if fold_minus_group_min <= D["pair"]["iqr"]
                         else "slower than the group_min launch"),
        "plan_minus_parent_us": plan_minus_parent,
        "plan_verdict": ("not slower than the parent's route" if plan_minus_parent <= H["plan"]["iqr"] + H["parent"]["iqr"]
                         else "slower than the parent's route"),
    }
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"step_{shape}.json"), "w") as f:
        json.dump(res, f, indent=1)
    brief = {"shape": shape, "form": form,
             "device_span_us": {k: [round(v["median"], 1), round(v["iqr"], 1)] for k, v in D.items()},
             "host_wall_us": {k: [round(v["median"], 1), round(v["iqr"], 1)] for k, v in H.items()},
             "fold_verdict": res["fold_verdict"], "plan_verdict": res["plan_verdict"]}
    print(json.dumps(brief), flush=True)
    return res


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", choices=sorted(SHAPES))
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "multiclass"))
    a = ap.parse_args()
    if a.rounds < 30:
        ap.error("--rounds must be at least 30")
    if a.shape is not None:
        run_shape(a.shape, a.rounds, a.out)
        return 0
    for shape in SHAPES:
        # a fresh process per shape, each under its own time limit; nothing
        # more is started on the GPU after a child fails or runs out of time
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", shape, "--rounds",
                                 str(a.rounds), "--out", a.out], timeout=CHILD_TIMEOUT_S).returncode
        except subprocess.TimeoutExpired:
            print(f"shape {shape}: no result within {CHILD_TIMEOUT_S} s; stopping", file=sys.stderr)
            return 124
        if rc != 0:
            print(f"shape {shape}: exit status {rc}; stopping", file=sys.stderr)
            return rc if rc > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
