// kernels_sankoff.h - weighted (Sankoff) parsimony (reference: src/parsimony.c:204-383) for gfx950.
//
// Layout. A score buffer holds, per site, one double per state: the cheapest cost of the subtree below the node given
// that the node shows that state. The reference keeps it [site][state]; in HBM it is tiled like the CLVs: a tile of 64
// sites as [state][64 lanes] doubles, tile after tile, so a lane owns a site and every row a wave reads or writes is one
// 512-byte line. The last tile is allocated in full; the lanes beyond the site count hold zeros after an upload and
// finite values afterwards, are computed like any other and never enter a sum or the host mirror. The [site][state] form
// exists only in the host mirror: k_sankoff_upload / k_sankoff_download transpose on the device.
//
// The step (src/parsimony.c:248-276), per site and parent state n:
//     parent[n] = min_k (child1[k] + M[k][n]) + min_k (child2[k] + M[k][n])
// A lane keeps the columns of both children in registers (2 x SMAX doubles, loaded before the first store: an operation
// whose parent is one of its own children is safe, no other lane touches the site) and walks the parent states in chunks
// of NCH: NCH running minima per child, the child states k unrolled. The cost matrix is wave-uniform and comes through
// the scalar path (as_const); on the device its rows are padded with zeros to a multiple of eight doubles, so a chunk
// never reads past a row. Only binary64 add and min (sp_min); every min runs over exactly the sums the reference forms
// (k = 0 initialises, k = 1 .. states-1 follow), so the buffers carry the reference's bits.
//
// Instantiations (sp_variant in pllgpu.hip): SMAX = 4 (NCH 4), 8, 24, 64 (NCH 8); the state count is a run-time value
// <= SMAX, the unrolled loops are cut by wave-uniform tests.
//
// Sums. A score is the sum over the sites of the per-site minimum. A lane adds the sites of its tiles in tile order,
// the wave reduces with shuffles, the workgroups hand their partials over through publish_candidate_sum
// (kernels_common.h): slots in index order, added by the workgroup that arrives last. Tiles per workgroup and the number
// of workgroups follow from the site count alone, so a sum has the same bits from run to run and - one set of slots and
// one ticket per candidate - whatever else the launch carries.
//
// No scalar-memory write of any kind: plain C++ stores and vector atomics.
#pragma once

#include <hip/hip_runtime.h>

#include "kernels_common.h"

constexpr unsigned kSpLanes = 64;       // one wave per workgroup: lane = site of a tile
constexpr unsigned kSpMaxBlocksY = 32768; // operations beyond it are walked with a grid stride

struct SpGeo
{
  unsigned states;
  unsigned sp;      // doubles per row of the padded cost matrix (states rounded up to 8)
  unsigned sites;
  unsigned tiles;   // (sites + 63) / 64
  size_t buf_doubles; // tiles * states * 64: one score buffer
};

struct SpOp
{
  unsigned parent, child1, child2;
};

struct SpPair
{
  unsigned a, b;
};

struct SpRecOp
{
  unsigned node_score, node_anc, parent_score, parent_anc; // ancestral indices count from the first ancestral buffer
  unsigned root;                                           // 1: the first operation of a call, reads no parent
};

// a lane's column of a tile: c[k] = row k of its site
template <int SMAX>
__device__ __forceinline__ void sp_load_column(const double *col, unsigned states, double (&c)[SMAX])
{
#pragma unroll
  for (int k = 0; k < SMAX; ++k) c[k] = (unsigned)k < states ? col[(size_t)k * kSpLanes] : 0.0;
}

// min as ONE v_min_f64. fmin() on a value that reaches it across a basic block - the running minimum, past the
// wave-uniform test on k - is preceded by a canonicalising v_max_f64 x, x: half as many binary64 instructions again in
// loops that consist of an add and a min. The instruction itself treats a NaN as fmin does (the other operand wins).
__device__ __forceinline__ double sp_min(double a, double b)
{
  double r;
  asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// r1[j] = min_k (c1[k] + M[k][n0 + j]) and the same for c2, j < NCH (src/parsimony.c:256-268)
template <int SMAX, int NCH>
__device__ __forceinline__ void sp_min_plus(const double (&c1)[SMAX], const double (&c2)[SMAX], cdouble_p m, unsigned sp, unsigned states,
                                            unsigned n0, double (&r1)[NCH], double (&r2)[NCH])
{
  cdouble_p row = m + n0;
#pragma unroll
  for (int j = 0; j < NCH; ++j)
  {
    const double w = row[j];
    r1[j] = c1[0] + w;
    r2[j] = c2[0] + w;
  }
#pragma unroll
  for (int k = 1; k < SMAX; ++k)
    if ((unsigned)k < states)
    {
      row = m + (size_t)k * sp + n0;
#pragma unroll
      for (int j = 0; j < NCH; ++j)
      {
        const double w = row[j];
        r1[j] = sp_min(c1[k] + w, r1[j]);
        r2[j] = sp_min(c2[k] + w, r2[j]);
      }
    }
}

// pll_parsimony_build for the operations of one dependency level: blockIdx.x = site tile, blockIdx.y (strided) = operation
template <int SMAX, int NCH>
__global__ __launch_bounds__(kSpLanes) void k_sankoff_build(double *buffers, const double *matrix, const SpOp *ops, unsigned nops, SpGeo g)
{
  const size_t at = (size_t)blockIdx.x * g.states * kSpLanes + threadIdx.x;
  cdouble_p m = as_const(matrix);
  for (unsigned o = blockIdx.y; o < nops; o += gridDim.y)
  {
    const SpOp op = ops[o];
    double c1[SMAX], c2[SMAX];
    sp_load_column<SMAX>(buffers + op.child1 * g.buf_doubles + at, g.states, c1);
    sp_load_column<SMAX>(buffers + op.child2 * g.buf_doubles + at, g.states, c2);
    double *p = buffers + op.parent * g.buf_doubles + at;
    for (unsigned n0 = 0; n0 < g.states; n0 += NCH)
    {
      double r1[NCH], r2[NCH];
      sp_min_plus<SMAX, NCH>(c1, c2, m, g.sp, g.states, n0, r1, r2);
#pragma unroll
      for (int j = 0; j < NCH; ++j)
        if (n0 + j < g.states) p[(size_t)(n0 + j) * kSpLanes] = r1[j] + r2[j];
    }
  }
}

// a lane's site minimum of a column in HBM (src/parsimony.c:297-304)
__device__ __forceinline__ double sp_site_min(const double *col, unsigned states)
{
  double mn = col[0];
  for (unsigned s = 1; s < states; ++s) mn = sp_min(col[(size_t)s * kSpLanes], mn);
  return mn;
}

// pll_parsimony_score: blockIdx.x (strided) = site tiles; the total lands in result[0]
__global__ __launch_bounds__(kSpLanes) void k_sankoff_score(const double *buffers, unsigned index, SpGeo g, double *block_sums, unsigned *ticket,
                                                            double *result, int fenced)
{
  const double *buf = buffers + index * g.buf_doubles + threadIdx.x;
  double acc = 0.0;
  for (unsigned t = blockIdx.x; t < g.tiles; t += gridDim.x)
  {
    const double mn = sp_site_min(buf + (size_t)t * g.states * kSpLanes, g.states);
    if (t * kSpLanes + threadIdx.x < g.sites) acc += mn;
  }
  publish_candidate_sum(block_sums, ticket, result, 0u, fenced, wave_sum(acc), 1u);
}

// pll_parsimony_reconstruct for the operations of one dependency level (src/parsimony.c:336-382): the first minimum of the
// node's column (strict <), kept against the parent's score at the parent's character unless the operation is the call's
// first. tables: revmap[256] (state -> character), then the state of each of the 256 characters (already < states).
// Ancestral buffers are [tiles * 64] words each: every lane of the last tile has a word of its own.
__global__ __launch_bounds__(kSpLanes) void k_sankoff_reconstruct(const double *buffers, unsigned *ancestral, const SpRecOp *ops, unsigned nops,
                                                                  const unsigned *tables, SpGeo g)
{
  const size_t at = (size_t)blockIdx.x * g.states * kSpLanes + threadIdx.x;
  const size_t site = (size_t)blockIdx.x * kSpLanes + threadIdx.x;
  const size_t anc_words = (size_t)g.tiles * kSpLanes;
  for (unsigned o = blockIdx.y; o < nops; o += gridDim.y)
  {
    const SpRecOp op = ops[o];
    const double *col = buffers + op.node_score * g.buf_doubles + at;
    double best = col[0];
    unsigned minindex = 0;
    for (unsigned s = 1; s < g.states; ++s)
    {
      const double v = col[(size_t)s * kSpLanes];
      if (v < best) best = v, minindex = s;
    }
    unsigned out = tables[minindex];
    if (!op.root)
    {
      const unsigned pchar = ancestral[op.parent_anc * anc_words + site];
      const unsigned pstate = tables[256u + (pchar & 255u)];
      const double parent_val = buffers[op.parent_score * g.buf_doubles + at + (size_t)pstate * kSpLanes];
      if (best + 1.0 > parent_val) out = pchar;
    }
    ancestral[op.node_anc * anc_words + site] = out;
  }
}

// Score of the tree obtained by inserting `node` into each candidate edge (a, b): what pll_parsimony_build returns for
// {{t1, a, b}, {t2, t1, node}}. t1's column goes through LDS ([state][lane], a lane reads back its own words), t2 is
// reduced to its minimum chunk by chunk and never exists. blockIdx.y = candidate, blockIdx.x (strided) = site tiles.
template <int SMAX, int NCH>
__global__ __launch_bounds__(kSpLanes) void k_sankoff_insertion(const double *buffers, const double *matrix, unsigned node, const SpPair *edges,
                                                                SpGeo g, double *block_sums, unsigned *tickets, double *results, int fenced)
{
  __shared__ double t1[SMAX * kSpLanes];
  const SpPair e = edges[blockIdx.y];
  cdouble_p m = as_const(matrix);
  double acc = 0.0;
  for (unsigned t = blockIdx.x; t < g.tiles; t += gridDim.x)
  {
    const size_t at = (size_t)t * g.states * kSpLanes + threadIdx.x;
    double c1[SMAX], c2[SMAX];
    sp_load_column<SMAX>(buffers + e.a * g.buf_doubles + at, g.states, c1);
    sp_load_column<SMAX>(buffers + e.b * g.buf_doubles + at, g.states, c2);
    for (unsigned n0 = 0; n0 < g.states; n0 += NCH)
    {
      double r1[NCH], r2[NCH];
      sp_min_plus<SMAX, NCH>(c1, c2, m, g.sp, g.states, n0, r1, r2);
#pragma unroll
      for (int j = 0; j < NCH; ++j)
        if (n0 + j < g.states) t1[(n0 + j) * kSpLanes + threadIdx.x] = r1[j] + r2[j];
    }
#pragma unroll
    for (int k = 0; k < SMAX; ++k) c1[k] = (unsigned)k < g.states ? t1[k * kSpLanes + threadIdx.x] : 0.0;
    sp_load_column<SMAX>(buffers + node * g.buf_doubles + at, g.states, c2);
    double best = 0.0;
    for (unsigned n0 = 0; n0 < g.states; n0 += NCH)
    {
      double r1[NCH], r2[NCH];
      sp_min_plus<SMAX, NCH>(c1, c2, m, g.sp, g.states, n0, r1, r2);
#pragma unroll
      for (int j = 0; j < NCH; ++j)
        if (n0 + j < g.states)
        {
          const double v = r1[j] + r2[j];
          best = n0 + j == 0 ? v : sp_min(v, best);
        }
    }
    if (t * kSpLanes + threadIdx.x < g.sites) acc += best;
  }
  publish_candidate_sum(block_sums, tickets, results, blockIdx.y, fenced, wave_sum(acc), 1u);
}

// host mirror -> tiles: staged[i] is buffer targets[i] as [site][state]; lanes beyond the site count store zeros.
// blockIdx.x = site tile, blockIdx.y = staged buffer
__global__ __launch_bounds__(kSpLanes) void k_sankoff_upload(double *buffers, const double *staged, const unsigned *targets, SpGeo g)
{
  const size_t site = (size_t)blockIdx.x * kSpLanes + threadIdx.x;
  const double *src = staged + (size_t)blockIdx.y * g.sites * g.states + site * g.states;
  double *dst = buffers + targets[blockIdx.y] * g.buf_doubles + (size_t)blockIdx.x * g.states * kSpLanes + threadIdx.x;
  const bool live = site < g.sites;
  for (unsigned s = 0; s < g.states; ++s) dst[(size_t)s * kSpLanes] = live ? src[s] : 0.0;
}

// tiles -> host mirror form
__global__ __launch_bounds__(kSpLanes) void k_sankoff_download(const double *buffers, double *staged, const unsigned *sources, SpGeo g)
{
  const size_t site = (size_t)blockIdx.x * kSpLanes + threadIdx.x;
  if (site >= g.sites) return;
  double *dst = staged + (size_t)blockIdx.y * g.sites * g.states + site * g.states;
  const double *src = buffers + sources[blockIdx.y] * g.buf_doubles + (size_t)blockIdx.x * g.states * kSpLanes + threadIdx.x;
  for (unsigned s = 0; s < g.states; ++s) dst[s] = src[(size_t)s * kSpLanes];
}
