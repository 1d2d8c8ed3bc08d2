// kernels_nj.h - neighbour-joining and BIONJ trees from a distance matrix (pll_gpu_nj_tree / pll_gpu_distance_tree,
// DESIGN.md section 5.16). pllamd/nj.py states the same operations in numpy, in the same order: it is the definition.
//
// count - 3 dependent steps of "find the pair of minimal Q, join it" over a matrix that shrinks by one node per step. The
// active nodes live in the slots 0 .. r-1 of a [count][count] working matrix D (BIONJ: a second one, V), both halves kept
// current; the row sums R and the slot -> label map ride along. A step is two launches on one stream:
//   k_nj_search  a workgroup takes rows w, w + gridDim.x, ... of the upper triangle, lanes along a row; the key
//                (Q, smaller label, larger label) is reduced across the wave, through LDS, to one partial per workgroup;
//                the workgroup that takes the last ticket reduces the partials (a minimum under a total order: the same
//                bits whoever arrives last) and leaves the step's record - the two slots, labels, d_ij, V_ij, R_i, R_j -
//                with a copy of rows i and j of D (and V), so that the join reads nothing it overwrites.
//   k_nj_join    a workgroup takes 256 values of k: d_uk (V_uk), R_k, row and column of the new node in slot i, the last
//                active slot moved into slot j (if i is the last slot, the new node takes j and nothing moves). BIONJ:
//                every workgroup forms lambda itself from the two copied V rows, in one fixed order. Workgroup 0 writes
//                the tree record, R_u and the labels.
// k_nj_init copies the upper triangle of the input into both halves of D (V) and forms the first row sums, k_nj_final
// joins the last three nodes. No workgroup ever waits for another: the only hand-off is the ticket, and the seams between
// search and join are launch boundaries.
//
// Several matrices of one size (pll_gpu_nj_trees, pll_gpu_bootstrap_distance_trees) are joined in
// lockstep: step s of every one has the same r, so the grids above get a second dimension, the replicate. Replicate b's
// working set - everything DevNj points at, its tickets, partials, record and status word included - lies `stride` bytes
// times b behind replicate 0's, its input `src_stride` doubles times b behind the first (nj_replicate). The last workgroup
// of a search is the last of its replicate: gridDim.x tickets per replicate and step.
//
// The row sums are carried forward (R_k <- R_k - d_ik - d_jk + d_uk); the first ones are added in slot order, one term at
// a time, by one thread per row. Q_ij = (r-2) d_ij - (R_i + R_j): the sum of the two row sums is formed first, so that Q
// is a function of the unordered pair. Every product is rounded before it is added.
#pragma once
#include "kernels_common.h"

struct NjKey
{
  double q;
  unsigned long long labels; // (smaller label << 32) | larger label: the tie rule is "<" on this word
  unsigned long long slots;  // (a << 32) | b, the pair's slots, a < b
};

struct NjRecord
{
  double dij, vij, ri, rj;
  unsigned si, sj; // slots of the pair; label li < lj
  unsigned li, lj;
};

struct DevNj
{
  double *D, *V;      // [count][count] working matrices (V: BIONJ, else null)
  double *R;          // [count] row sums by slot
  double *snap;       // [4][count]: rows i and j of D, then of V, as the search left them
  unsigned *label;    // [count] slot -> label
  unsigned *tickets;  // [count] one per step, zero before the first launch
  NjKey *partials;    // [search workgroups]
  NjRecord *record;   // the current step's
  int *parent;        // [2 count - 2]
  double *length;     // [2 count - 2]
  unsigned *status;   // != 0: a step found no pair (a criterion that is not a number)
  size_t stride;      // bytes from a replicate's working set to the next one's
  size_t src_stride;  // doubles from a replicate's input matrix to the next one's
  unsigned count;
  unsigned rows;      // rows of the triangle per search workgroup
  unsigned bionj;
};

// replicate b's working set: every pointer of replicate 0's, b strides further on
__device__ __forceinline__ DevNj nj_replicate(const DevNj &base, unsigned b)
{
  DevNj n = base;
  const size_t off = (size_t)b * base.stride;
  auto shift = [off](auto *p) { return reinterpret_cast<decltype(p)>(reinterpret_cast<unsigned char *>(p) + off); };
  n.D = shift(base.D);
  n.V = base.V ? shift(base.V) : nullptr;
  n.R = shift(base.R);
  n.snap = shift(base.snap);
  n.label = shift(base.label);
  n.tickets = shift(base.tickets);
  n.partials = shift(base.partials);
  n.record = shift(base.record);
  n.parent = shift(base.parent);
  n.length = shift(base.length);
  n.status = shift(base.status);
  return n;
}

__device__ __forceinline__ bool nj_before(double q, unsigned long long labels, const NjKey &y)
{
  return q < y.q || (q == y.q && labels < y.labels);
}

__device__ __forceinline__ void nj_take(NjKey &best, double q, unsigned long long labels, unsigned long long slots)
{
  const bool better = nj_before(q, labels, best);
  best.q = better ? q : best.q;
  best.labels = better ? labels : best.labels;
  best.slots = better ? slots : best.slots;
}

__device__ __forceinline__ NjKey nj_none()
{
  NjKey k;
  k.q = __builtin_inf();
  k.labels = k.slots = ~0ull;
  return k;
}

// the workgroup's minimum in thread 0 (every thread of the workgroup calls)
__device__ __forceinline__ NjKey nj_workgroup_min(NjKey k, NjKey *ws)
{
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
  {
    const double q = __shfl_down(k.q, off, 64);
    const unsigned long long labels = __shfl_down(k.labels, off, 64), slots = __shfl_down(k.slots, off, 64);
    nj_take(k, q, labels, slots);
  }
  __syncthreads(); // (ws may still be read from the previous call)
  if (lane == 0) ws[wave] = k;
  __syncthreads();
  if (threadIdx.x == 0)
    for (unsigned w = 1; w < nw; ++w) nj_take(k, ws[w].q, ws[w].labels, ws[w].slots);
  return k;
}

// src: [count][count], only [x][y] with x < y is read. One workgroup per row x: both halves of D (and V) from the upper
// triangle, the diagonal 0, label[x] = x; thread 0 adds the row's sum in slot order.
__global__ __launch_bounds__(256) void k_nj_init(const DevNj base, const double *__restrict__ src0)
{
  const DevNj n = nj_replicate(base, blockIdx.y);
  const double *__restrict__ src = src0 + (size_t)blockIdx.y * base.src_stride;
  const unsigned x = blockIdx.x, c = n.count;
  for (unsigned y = threadIdx.x; y < c; y += blockDim.x)
  {
    const double d = x == y ? 0.0 : src[(size_t)min(x, y) * c + max(x, y)];
    n.D[(size_t)x * c + y] = d;
    if (n.V) n.V[(size_t)x * c + y] = d;
  }
  if (threadIdx.x == 0)
  {
    double s = 0.0;
    for (unsigned y = 0; y < c; ++y) s += x == y ? 0.0 : src[(size_t)min(x, y) * c + max(x, y)];
    n.R[x] = s;
    n.label[x] = x;
  }
}

__global__ __launch_bounds__(256) void k_nj_search(const DevNj base, unsigned r, unsigned step)
{
#pragma clang fp contract(off)
  const DevNj n = nj_replicate(base, blockIdx.y);
  __shared__ NjKey ws[4];
  __shared__ unsigned last;
  __shared__ NjRecord rec;
  const unsigned c = n.count;
  const double rm2 = (double)(r - 2u);
  // four nodes left: Q_ab = Q_cd for every split, so only the pairs of the active node with the smallest label
  unsigned only = 0xffffffffu;
  if (r == 4u)
  {
    only = 0u;
    for (unsigned s = 1; s < 4u; ++s)
      if (n.label[s] < n.label[only]) only = s;
  }
  NjKey best = nj_none();
  for (unsigned t = 0; t < n.rows; ++t)
  {
    const unsigned a = blockIdx.x + t * gridDim.x;
    if (a + 1u >= r) break;
    const double ra = n.R[a];
    const unsigned la = n.label[a];
    const double *row = n.D + (size_t)a * c;
    for (unsigned b = a + 1u + threadIdx.x; b < r; b += blockDim.x)
    {
      if (only != 0xffffffffu && a != only && b != only) continue;
      const unsigned lb = n.label[b];
      const unsigned lo = la < lb ? la : lb, hi = la < lb ? lb : la;
      nj_take(best, rm2 * row[b] - (ra + n.R[b]), ((unsigned long long)lo << 32) | hi, ((unsigned long long)a << 32) | b);
    }
  }
  best = nj_workgroup_min(best, ws);
  if (threadIdx.x == 0)
  {
    NjKey *slot = n.partials + blockIdx.x;
    __hip_atomic_store(&slot->q, best.q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&slot->labels, best.labels, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&slot->slots, best.slots, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // release: the partial is visible to whoever reads the ticket after this; acquire: the last one sees them all
    const unsigned ticket = __hip_atomic_fetch_add(n.tickets + step, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    last = ticket == gridDim.x - 1u ? 1u : 0u;
  }
  __syncthreads();
  if (!last) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  best = nj_none();
  for (unsigned w = threadIdx.x; w < gridDim.x; w += blockDim.x)
  {
    const NjKey *slot = n.partials + w;
    const double q = __hip_atomic_load(&slot->q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long labels = __hip_atomic_load(&slot->labels, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long slots = __hip_atomic_load(&slot->slots, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    nj_take(best, q, labels, slots);
  }
  best = nj_workgroup_min(best, ws);
  if (threadIdx.x == 0)
  {
    NjRecord q = {};
    q.si = q.sj = 0xffffffffu; // no pair: the join does nothing and the call fails
    const unsigned a = (unsigned)(best.slots >> 32), b = (unsigned)best.slots;
    if (a < r && b < r && a != b)
    {
      const bool a_first = n.label[a] < n.label[b];
      q.si = a_first ? a : b;
      q.sj = a_first ? b : a;
      q.li = (unsigned)(best.labels >> 32);
      q.lj = (unsigned)best.labels;
      q.dij = n.D[(size_t)q.si * c + q.sj];
      q.vij = n.V ? n.V[(size_t)q.si * c + q.sj] : 0.0;
      q.ri = n.R[q.si];
      q.rj = n.R[q.sj];
    }
    else
      *n.status = 1u;
    rec = q;
    *n.record = q;
  }
  __syncthreads();
  if (rec.si >= r) return;
  const double *di = n.D + (size_t)rec.si * c, *dj = n.D + (size_t)rec.sj * c;
  for (unsigned k = threadIdx.x; k < r; k += blockDim.x)
  {
    n.snap[k] = di[k];
    n.snap[c + k] = dj[k];
  }
  if (n.V)
  {
    const double *vi = n.V + (size_t)rec.si * c, *vj = n.V + (size_t)rec.sj * c;
    for (unsigned k = threadIdx.x; k < r; k += blockDim.x)
    {
      n.snap[2u * c + k] = vi[k];
      n.snap[3u * c + k] = vj[k];
    }
  }
}

// lambda of BIONJ: the sum of V_jk - V_ik over the slots k other than i and j (a 0.0 stands in their places), thread t
// adding k = t, t + 256, ... in that order, then the wave's 64 values by halving (lane l takes l + 32, l + 16, ...), then
// the four waves in order; pllamd/nj.py adds in the same order.
__device__ __forceinline__ double nj_lambda(const DevNj &n, const NjRecord &q, unsigned r, double *ws)
{
#pragma clang fp contract(off)
  const unsigned c = n.count;
  const double *vi = n.snap + 2u * c, *vj = n.snap + 3u * c;
  double s = 0.0;
  for (unsigned k = threadIdx.x; k < r; k += blockDim.x) s += (k == q.si || k == q.sj) ? 0.0 : vj[k] - vi[k];
  s = wave_sum(s);
  if ((threadIdx.x & 63u) == 0) ws[threadIdx.x >> 6] = s;
  __syncthreads();
  const double total = ((ws[0] + ws[1]) + ws[2]) + ws[3];
  if (q.vij == 0.0) return 0.5;
  double lambda = 0.5 + total / (2.0 * (double)(r - 2u) * q.vij);
  if (!(lambda >= 0.0)) lambda = 0.0;
  if (lambda > 1.0) lambda = 1.0;
  return lambda;
}

__global__ __launch_bounds__(256) void k_nj_join(const DevNj base, unsigned r, unsigned step)
{
#pragma clang fp contract(off)
  const DevNj n = nj_replicate(base, blockIdx.y);
  __shared__ double ws[4];
  const NjRecord q = *n.record;
  if (q.si >= r || q.sj >= r || q.si == q.sj) return; // the search found no pair (status says so)
  const unsigned c = n.count, lastslot = r - 1u;
  const double rm2 = (double)(r - 2u);
  const double len_i = 0.5 * q.dij + (q.ri - q.rj) / (2.0 * rm2);
  const double len_j = q.dij - len_i;
  double lambda = 0.5;
  if (n.bionj) lambda = nj_lambda(n, q, r, ws);
  const double mu = 1.0 - lambda;
  // where things go: the new node into slot i and the last slot into slot j - or, when i is the last slot, into j
  const unsigned su = q.si == lastslot ? q.sj : q.si;
  const bool move = q.si != lastslot && q.sj != lastslot;
  const unsigned u = c + step;
  if (blockIdx.x == 0 && threadIdx.x == 0)
  {
    n.parent[q.li] = (int)u;
    n.parent[q.lj] = (int)u;
    n.length[q.li] = len_i;
    n.length[q.lj] = len_j;
    double ru;
    if (n.bionj)
    {
      const double ru_i = (q.ri - q.dij) - rm2 * len_i, ru_j = (q.rj - q.dij) - rm2 * len_j;
      ru = ru_j + lambda * (ru_i - ru_j);
    }
    else
      ru = 0.5 * ((q.ri + q.rj) - (double)r * q.dij);
    n.R[su] = ru;
    n.label[su] = u;
    n.D[(size_t)su * c + su] = 0.0;
    if (n.V) n.V[(size_t)su * c + su] = 0.0;
  }
  const unsigned k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= r || k == q.si || k == q.sj) return;
  const double dik = n.snap[k], djk = n.snap[c + k];
  double duk, vuk = 0.0;
  if (n.bionj)
  {
    const double vik = n.snap[2u * c + k], vjk = n.snap[3u * c + k];
    duk = (djk - len_j) + lambda * ((dik - len_i) - (djk - len_j)); // exact where both sides agree (an additive matrix)
    vuk = (lambda * vik + mu * vjk) - (lambda * mu) * q.vij;
  }
  else
    duk = 0.5 * ((dik + djk) - q.dij);
  const double rk = ((n.R[k] - dik) - djk) + duk;
  const unsigned kn = (move && k == lastslot) ? q.sj : k; // the slot k has after this step
  if (move && k != lastslot)
  {
    // the last slot's row and column into slot j (row lastslot is written by nobody in this launch)
    const double m = n.D[(size_t)lastslot * c + k];
    n.D[(size_t)q.sj * c + k] = m;
    n.D[(size_t)k * c + q.sj] = m;
    if (n.V)
    {
      const double mv = n.V[(size_t)lastslot * c + k];
      n.V[(size_t)q.sj * c + k] = mv;
      n.V[(size_t)k * c + q.sj] = mv;
    }
  }
  if (move && k == lastslot)
  {
    n.label[q.sj] = n.label[lastslot];
    n.D[(size_t)q.sj * c + q.sj] = 0.0;
    if (n.V) n.V[(size_t)q.sj * c + q.sj] = 0.0;
  }
  n.D[(size_t)su * c + kn] = duk;
  n.D[(size_t)kn * c + su] = duk;
  if (n.V)
  {
    n.V[(size_t)su * c + kn] = vuk;
    n.V[(size_t)kn * c + su] = vuk;
  }
  n.R[kn] = rk;
}

// the last three nodes, in the slots 0, 1, 2 of a matrix (only [x][y], x < y, is read): one thread per replicate. src ==
// null: the working matrix and its labels. Else the replicate's input matrix, the slots being the labels (count == 3:
// nothing ran before).
__global__ void k_nj_final(const DevNj base, const double *__restrict__ src)
{
#pragma clang fp contract(off)
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const DevNj n = nj_replicate(base, blockIdx.y);
  const double *d = src ? src + (size_t)blockIdx.y * base.src_stride : n.D;
  const unsigned *label = src ? nullptr : n.label;
  const unsigned c = n.count, root = 2u * c - 3u;
  const double d01 = d[1], d02 = d[2], d12 = d[c + 2u];
  const unsigned l0 = label ? label[0] : 0u, l1 = label ? label[1] : 1u, l2 = label ? label[2] : 2u;
  n.parent[l0] = n.parent[l1] = n.parent[l2] = (int)root;
  n.length[l0] = 0.5 * ((d01 + d02) - d12);
  n.length[l1] = 0.5 * ((d01 + d12) - d02);
  n.length[l2] = 0.5 * ((d02 + d12) - d01);
  n.parent[root] = -1;
  n.length[root] = 0.0;
}
