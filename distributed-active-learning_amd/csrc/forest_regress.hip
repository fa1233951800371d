// Regression forests: RandomForestModel.predict of a regression model, the
// mean of the trees' real-valued leaves.
//
// Reference:
//   lal_direct_mllib_implementation/classes/active_learner.py:319
//       self.lalModel.predict(LALDataset.map(lambda _: _.features))
//   :354-365  RandomForest.trainRegressor(reg, numTrees=2000, ...) / RandomForestModel.load
//   MLlib 2.1 RandomForestModel (TreeEnsembleModel.predictBySumming, Average):
//       trees.map(_.predict(features)).sum / numTrees
//   Node.predict: continuous split, features(f) <= threshold -> left.
//
// Canonical value of a row r (include/dal.h):
//   R(r) = (((0.0 + leaf_0(r)) + leaf_1(r)) + ... + leaf_{TR-1}(r)) / (double)TR
// a sequential fp64 chain in tree order.  fp64 addition is not associative, so
// a row is owned by ONE lane from the first tree to the last: trees are never
// split across lanes, waves or blocks, and no floating-point atomics exist
// here.  What is parallel inside a lane is the tree WALKS: kRegIlp trees of a
// chunk are walked interleaved (their dependent LDS round trips overlap, as
// the binary kernel's M-way walk does) and their leaves are then added in
// tree order.
//
// MI355X design.  A block of 256 threads keeps a tile of 256 rows (one per
// lane) and streams the forest through LDS in chunks of
// dal_forest_regress_chunk_trees(depth) trees: 2,000 depth-4 trees are 736 KB
// of 16-byte nodes and 8-byte leaves, far above the CU's 160 KiB.
//   nodes   {fp64 threshold, int32 feature, pad}: one ds_read_b128 per visit
//   leaves  fp64: one ds_read_b64 per tree
//   rows    feature-major fp64 xs[f][256] when d <= kRegXLdsFeatures: lane l
//           reads xs[f_l][l], bank (2 l) mod 64 whatever f_l -- conflict-free
//           inside each 32-lane group; wider rows are read from global memory
// Chunk (40 KiB) + row tile (<= 20 KiB) stay under 64 KiB, so two blocks share
// a CU; a block loads its next chunk into registers under the current chunk's
// walks (ChunkRegs) and moves it to LDS between two barriers.
// The thresholds are the model's fp64 values and the compare is fp64: LAL's
// feature rows (v/T, an SD, ...) are not fp32-representable, so the classifier
// kernels' "threshold rounded toward -inf to fp32" does not apply.  An fp32
// row is widened exactly, (double)x <= threshold.  A NaN feature compares
// false and goes right, as in the JVM.
#include "common.hpp"

namespace dal {
namespace {

constexpr int kRegThreads = 256;             // rows per block: one per lane
#ifndef DAL_REG_ILP
#define DAL_REG_ILP 16  // (8: the one-block LAL launch 302 us instead of 270; the pool launch the same)
#endif
constexpr int kRegIlp = DAL_REG_ILP;         // tree walks in flight per lane
constexpr int kRegChunkBytes = 40 * 1024;    // LDS for one chunk of trees
constexpr int kRegXLdsFeatures = 10;         // row tile in LDS up to this d (20 KiB of fp64)

struct __attribute__((aligned(16))) RegNode {
  double thr;
  int feat;
  int pad;
};

__host__ __device__ constexpr int reg_tree_bytes(int depth) {
  return ((1 << depth) - 1) * static_cast<int>(sizeof(RegNode)) + (1 << depth) * static_cast<int>(sizeof(double));
}

// Trees per chunk: what fits kRegChunkBytes, a multiple of kRegIlp when that
// many fit (whole walk groups), at least one.
__host__ __device__ constexpr int reg_chunk_trees(int depth) {
  const int c = kRegChunkBytes / reg_tree_bytes(depth);
  return c >= kRegIlp ? c / kRegIlp * kRegIlp : (c < 1 ? 1 : c);
}
static_assert(reg_tree_bytes(DAL_REG_MAX_DEPTH) <= kRegChunkBytes, "one tree of the maximum depth fits a chunk");

struct RegArgs {
  const void* x;
  int64_t n;
  int d;
  int64_t ldx;
  const int32_t* feat;
  const double* thr;
  const double* leaf;
  int n_trees;
  int depth;
  double* out;
};

// M trees t0 .. t0 + M - 1 of the chunk walked together for this lane's row,
// their leaves added to the running sum in tree order.
template <int M, bool X_LDS, class XT>
__device__ __forceinline__ double walk_add(double sum, const RegNode* nodes, const double* leaves, int t0,
                                           int n_inner, int n_leaf, int depth, const double* xs, const XT* xrow) {
  int h[M];
#pragma unroll
  for (int j = 0; j < M; ++j) h[j] = 0;
  for (int lvl = 0; lvl < depth; ++lvl) {
    // a level is two dependent round trips, whatever M: the M node reads
    // together, then the M feature reads together
    RegNode nd[M];
    double xv[M];
#pragma unroll
    for (int j = 0; j < M; ++j) nd[j] = nodes[(t0 + j) * n_inner + h[j]];
#pragma unroll
    for (int j = 0; j < M; ++j) xv[j] = X_LDS ? xs[nd[j].feat * kRegThreads] : static_cast<double>(xrow[nd[j].feat]);
#pragma unroll
    for (int j = 0; j < M; ++j) h[j] = 2 * h[j] + (xv[j] <= nd[j].thr ? 1 : 2);
  }
  double lv[M];
#pragma unroll
  for (int j = 0; j < M; ++j) lv[j] = leaves[(t0 + j) * n_leaf + (h[j] - n_inner)];
#pragma unroll
  for (int j = 0; j < M; ++j) sum = __dadd_rn(sum, lv[j]);  // tree order, one rounding per add
  return sum;
}

// A thread's share of one chunk, held in registers between its global loads
// and its LDS stores: item j of the thread is element tid + j * 256 of the
// chunk's nodes (leaves).  The loads of chunk c + 1 are issued before the
// walks of chunk c and stored after them, so a block -- the LAL step runs ONE
// block, 2,000 depth-4 trees in 21 chunks -- does not sit out a global round trip per
// staging iteration between chunks.
constexpr int kRegNodeRegs = 8;
constexpr int kRegLeafRegs = 10;
constexpr bool reg_regs_hold_a_chunk() {
  for (int depth = 1; depth <= DAL_REG_MAX_DEPTH; ++depth) {
    const int c = reg_chunk_trees(depth);
    if (c * ((1 << depth) - 1) > kRegNodeRegs * kRegThreads || c * (1 << depth) > kRegLeafRegs * kRegThreads)
      return false;
  }
  return true;
}
static_assert(reg_regs_hold_a_chunk(), "a chunk's nodes and leaves fit the threads' prefetch registers at every depth");

struct ChunkRegs {
  double thr[kRegNodeRegs];
  int feat[kRegNodeRegs];
  double leaf[kRegLeafRegs];

  __device__ __forceinline__ void load(const RegArgs& A, int c0, int ct, int n_inner, int n_leaf, int tid) {
    const int64_t nb = static_cast<int64_t>(c0) * n_inner, lb = static_cast<int64_t>(c0) * n_leaf;
#pragma unroll
    for (int j = 0; j < kRegNodeRegs; ++j) {
      const int i = tid + j * kRegThreads;
      if (i < ct * n_inner) {
        thr[j] = A.thr[nb + i];
        feat[j] = A.feat[nb + i];
      }
    }
#pragma unroll
    for (int j = 0; j < kRegLeafRegs; ++j) {
      const int i = tid + j * kRegThreads;
      if (i < ct * n_leaf) leaf[j] = A.leaf[lb + i];
    }
  }

  __device__ __forceinline__ void store(RegNode* nodes, double* leaves, int ct, int n_inner, int n_leaf, int tid,
                                        int d) const {
#pragma unroll
    for (int j = 0; j < kRegNodeRegs; ++j) {
      const int i = tid + j * kRegThreads;
      if (i < ct * n_inner) {
        RegNode nd;
        nd.thr = thr[j];
        nd.feat = feat[j] < 0 ? 0 : feat[j] >= d ? d - 1 : feat[j];  // (outside [0, d): the caller's error; no stray read)
        nd.pad = 0;
        nodes[i] = nd;
      }
    }
#pragma unroll
    for (int j = 0; j < kRegLeafRegs; ++j) {
      const int i = tid + j * kRegThreads;
      if (i < ct * n_leaf) leaves[i] = leaf[j];
    }
  }
};

template <bool X_LDS, class XT>
__global__ __launch_bounds__(kRegThreads) void forest_regress_kernel(RegArgs A, int chunk) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int n_inner = (1 << A.depth) - 1;
  const int n_leaf = 1 << A.depth;
  RegNode* nodes = reinterpret_cast<RegNode*>(smem);
  double* leaves = reinterpret_cast<double*>(smem + static_cast<size_t>(chunk) * n_inner * sizeof(RegNode));
  double* xs = leaves + static_cast<size_t>(chunk) * n_leaf;  // [d][256], X_LDS only

  const int tid = threadIdx.x;
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * kRegThreads;
  const int64_t row = row0 + tid;
  const bool live = row < A.n;
  const XT* xg = static_cast<const XT*>(A.x);

  if (X_LDS) {
    // coalesced over the tile's rows (contiguous when ldx == d), feature-major in LDS
    const int rows = static_cast<int>(A.n - row0 < kRegThreads ? A.n - row0 : kRegThreads);
    for (int i = tid; i < kRegThreads * A.d; i += kRegThreads) {
      const int r = i / A.d, f = i - r * A.d;
      xs[f * kRegThreads + r] = r < rows ? static_cast<double>(xg[(row0 + r) * A.ldx + f]) : 0.0;
    }
  }
  const XT* xrow = xg + (live ? row : 0) * A.ldx;

  double sum = 0.0;
  ChunkRegs next;
  next.load(A, 0, A.n_trees < chunk ? A.n_trees : chunk, n_inner, n_leaf, tid);
  for (int c0 = 0; c0 < A.n_trees; c0 += chunk) {
    const int ct = A.n_trees - c0 < chunk ? A.n_trees - c0 : chunk;
    __syncthreads();  // the previous chunk's walks are done
    next.store(nodes, leaves, ct, n_inner, n_leaf, tid, A.d);
    __syncthreads();
    // the next chunk's global loads fly under this chunk's walks
    const int c1 = c0 + chunk;
    if (c1 < A.n_trees) next.load(A, c1, A.n_trees - c1 < chunk ? A.n_trees - c1 : chunk, n_inner, n_leaf, tid);
    if (live) {
      int t = 0;
      for (; t + kRegIlp <= ct; t += kRegIlp)
        sum = walk_add<kRegIlp, X_LDS>(sum, nodes, leaves, t, n_inner, n_leaf, A.depth, xs + tid, xrow);
      if (kRegIlp > 8 && t + 8 <= ct) {
        sum = walk_add<8, X_LDS>(sum, nodes, leaves, t, n_inner, n_leaf, A.depth, xs + tid, xrow);
        t += 8;
      }
      if (t + 4 <= ct) {
        sum = walk_add<4, X_LDS>(sum, nodes, leaves, t, n_inner, n_leaf, A.depth, xs + tid, xrow);
        t += 4;
      }
      if (t + 2 <= ct) {
        sum = walk_add<2, X_LDS>(sum, nodes, leaves, t, n_inner, n_leaf, A.depth, xs + tid, xrow);
        t += 2;
      }
      if (t < ct) sum = walk_add<1, X_LDS>(sum, nodes, leaves, t, n_inner, n_leaf, A.depth, xs + tid, xrow);
    }
  }
  if (live) A.out[row] = sum / static_cast<double>(A.n_trees);  // one IEEE division
}

template <class XT>
int regress_launch(const RegArgs& A, hipStream_t st) {
  const int chunk = reg_chunk_trees(A.depth);
  const bool x_lds = A.d <= kRegXLdsFeatures;
  const size_t smem = static_cast<size_t>(chunk) * reg_tree_bytes(A.depth) +
                      (x_lds ? static_cast<size_t>(A.d) * kRegThreads * sizeof(double) : 0);
  const dim3 grid(static_cast<unsigned>(ceil_div(A.n, kRegThreads)));
  if (x_lds)
    hipLaunchKernelGGL((forest_regress_kernel<true, XT>), grid, dim3(kRegThreads), smem, st, A, chunk);
  else
    hipLaunchKernelGGL((forest_regress_kernel<false, XT>), grid, dim3(kRegThreads), smem, st, A, chunk);
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}

}  // namespace
}  // namespace dal

using namespace dal;

extern "C" int dal_forest_regress_chunk_trees(int32_t depth) {
  if (depth < 1 || depth > DAL_REG_MAX_DEPTH) return 0;
  return reg_chunk_trees(depth);
}

extern "C" int dal_forest_regress(const void* x, int x_dtype, int64_t n, int64_t d, int64_t ldx,
                                  const int32_t* inner_feature, const double* inner_threshold, const double* leaf,
                                  int32_t n_trees, int32_t depth, double* out, dal_stream_t stream) {
  if (!x || !inner_feature || !inner_threshold || !leaf || !out) return DAL_ERR_ARG;
  if (x_dtype != DAL_X_F32 && x_dtype != DAL_X_F64) return DAL_ERR_ARG;
  if (depth < 1 || depth > DAL_REG_MAX_DEPTH) return DAL_ERR_UNSUPPORTED;
  if (n_trees < 1) return DAL_ERR_SHAPE;
  if (n < 0 || d < 1 || ldx < d || d > (int64_t{1} << 24)) return DAL_ERR_SHAPE;
  if (ceil_div(n, kRegThreads) > INT32_MAX) return DAL_ERR_SHAPE;
  if (n == 0) return DAL_OK;
  const RegArgs A{x, n, static_cast<int>(d), ldx, inner_feature, inner_threshold, leaf, n_trees, depth, out};
  return x_dtype == DAL_X_F32 ? regress_launch<float>(A, as_stream(stream))
                              : regress_launch<double>(A, as_stream(stream));
}
