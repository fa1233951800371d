"""The thresholded pair filter (dal_cosine_pairs) and, for comparison, the
density Gram's MFMA launches at one shape, a few launches each, for
rocprofv3 --pmc (counters only, one counter group per run).
usage: python scripts/pairs_pmc.py NxD [reps] [tau]"""
import os
import sys

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(REPO, "distributed-active-learning_amd"))
sys.path.insert(0, REPO)
import torch  # noqa: E402

import bench  # noqa: E402
from dal import similarity as sim  # noqa: E402
from dal.engine import PoolState  # noqa: E402

dev = torch.device("cuda:0")
n, d = (int(v) for v in sys.argv[1].split("x"))
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 2
tau = float(sys.argv[3]) if len(sys.argv) > 3 else 0.85
st = PoolState(bench.upload(bench.host_pool(0, n, d, "normal" if d == 30 else "uniform"), dev), device=dev)
op = st.gram_operand()
acc = torch.zeros(st.n_pad, dtype=torch.int64, device=dev)
for _ in range(reps):
    keys, approx, count, status = sim.cosine_pair_candidates(st, tau, 1 << 20)
    acc.zero_()
    st.gram_accumulate(acc, op, st.n_pad)
torch.cuda.synchronize()
print("ok", n, d, reps, int(count.item()), int(status.item()))
