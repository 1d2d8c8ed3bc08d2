// kernels_placement.h - batched placement log-likelihoods (pll_gpu_placement_loglikelihoods).
//
// "What is the log-likelihood if query tip q is inserted into edge (a, b)?" for every query x every candidate edge. The
// candidates, the model and the pendant matrix are the insertion kernels' (kernels_insertion.h); only the subtree end
// changes between two queries, and it is one byte per site. So the inserted node of a candidate - both ends read, the
// products, the scaling decision - is formed ONCE per site tile and stays in registers (4 x 4) or LDS (every other
// shape) while a chunk of QCH queries is scored against it, each into an accumulator of its own.
//
// Grid: x = the site tiles exactly as the insertion kernels cut them, y = the candidate, z = the chunk of QCH queries.
// Per (query, candidate) the arithmetic of a site, the order of the lane's sum over its tiles, the wave sum and the
// hand-off (publish_candidate_sum's steps, one slot per workgroup, one ticket per pair: plc_publish_chunk) are
// k_insertion_dna's / k_insertion_tiled's with a tip as the subtree end, call for call: a pair's value has the bits
// pllgpu_insertion_loglikelihoods gives it.
//
// DevEdge: mat = the pendant matrix; block_sums = [query of the launch][candidate of the launch][workgroup] partial
// slots; counter = one ticket per (query, candidate) of the launch; result = the (first query, first candidate) of the
// launch in the call's [query][candidate] matrix, rows `res_stride` apart. qrows = the code rows of the launch's nq
// queries, read through the scalar path.
#pragma once
#include "kernels_insertion.h"

constexpr int kPlcDnaChunk = 16;  // queries per workgroup, 4 x 4 (register report in DESIGN.md section 5.7)
constexpr int kPlcTiledChunk = 4; // ... every other shape: 7 KB of LDS per query beside the node tile

typedef const unsigned char *const __attribute__((address_space(4))) *cqrow_p;

__device__ __forceinline__ const unsigned char *plc_row(const unsigned char *const *qrows, unsigned q)
{
  return ((cqrow_p)(uintptr_t)qrows)[q];
}

// The hand-off of a chunk: pair (query q0 + j of the launch, candidate blockIdx.y) has its slots, its ticket and its place
// in the result matrix, and the workgroup holds a value for each of the nqh pairs. These are handoff_block_sum's steps
// (kernels_common.h) per pair - the waves' values added in wave order, the partial performed before the ticket is taken,
// the pair's last workgroup adding the slots with sum_partials_strided / wave_sum and leaving the ticket at zero - so a
// pair's total has the bits publish_candidate_sum gives it. What differs is that thread j serves pair j: the nqh
// stores, waits and tickets travel side by side instead of nqh round trips to the coherent level one after the other,
// which is where a workgroup of one tile per wave would otherwise spend its life.
template <int QCH>
__device__ __forceinline__ void plc_publish_chunk(const DevEdge &e, unsigned q0, unsigned nqh, unsigned res_stride, const double (&wave_value)[QCH],
                                                  unsigned nsum_waves)
{
  static_assert(QCH <= 32, "one bit per pair of the chunk");
  __shared__ double ws[QCH][4];
  __shared__ unsigned last_pairs;
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if (lane == 0)
  {
#pragma unroll
    for (int j = 0; j < QCH; ++j) ws[j][wave] = wave < nsum_waves ? wave_value[j] : 0.0;
  }
  if (threadIdx.x == 0) last_pairs = 0u;
  __syncthreads();
  if (threadIdx.x < nqh)
  {
    const unsigned j = threadIdx.x;
    const size_t pair = (size_t)(q0 + j) * gridDim.y + blockIdx.y;
    double s = ws[j][0];
    for (unsigned w = 1; w < nw; ++w) s += ws[j][w];
    partial_store(&e.block_sums[pair * gridDim.x + blockIdx.x], s);
    handoff_before_ticket(e.fenced); // the partial has been performed before the ticket is taken
    const unsigned ticket = __hip_atomic_fetch_add(e.counter + pair, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (ticket == gridDim.x - 1)
    {
      handoff_after_last_ticket(e.fenced);
      atomicOr(&last_pairs, 1u << j);
    }
  }
  __syncthreads();
  unsigned todo = __builtin_amdgcn_readfirstlane(last_pairs); // the pairs this workgroup arrived last at (workgroup-uniform)
  while (todo)
  {
    const unsigned j = __builtin_ctz(todo);
    todo &= todo - 1u;
    const size_t pair = (size_t)(q0 + j) * gridDim.y + blockIdx.y;
    double a = sum_partials_strided(e.block_sums + pair * gridDim.x, gridDim.x);
    a = wave_sum(a);
    if (lane == 0) ws[0][wave] = a; // (ws was last read before the barrier above, or before the one that ends the previous round)
    __syncthreads();
    if (threadIdx.x == 0)
    {
      double s = ws[0][0];
      for (unsigned w = 1; w < nw; ++w) s += ws[0][w];
      __hip_atomic_store(e.counter + pair, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      e.result[(size_t)(q0 + j) * res_stride + blockIdx.y] = s; // read by the copy that follows the kernel on the stream
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------
// 4 states x 4 rates: one wave per 64-site tile as k_insertion_dna. The inserted node's v[4][4], its scaler words and
// the site's scaling counts (a tip end adds none) are computed once per tile; per query one byte per lane, the tip's
// column sums of the pendant matrix and the site mix.
template <int QCH>
__global__ __launch_bounds__(256) void k_placement_dna(const DevEdge e, const InsCand *cands, const unsigned char *const *qrows, unsigned nq,
                                                       unsigned res_stride, int scale_mode, unsigned tiles_per_wave)
{
  const InsCand c = ins_get(cands, blockIdx.y);
  InsOp op;
  op.lmat = c.lmat;
  op.rmat = c.rmat;
  op.pscaler = true;
  cdouble_p pm = as_const(e.mat);
  const unsigned q0 = blockIdx.z * QCH;
  const unsigned nqh = min((unsigned)QCH, nq - q0); // queries of this chunk (workgroup-uniform)
  const unsigned char *row[QCH];                    // (past the chunk's end: the last query's row again, read and not used)
#pragma unroll
  for (int j = 0; j < QCH; ++j) row[j] = plc_row(qrows, q0 + min((unsigned)j, nqh - 1u));
  double acc[QCH];
#pragma unroll
  for (int j = 0; j < QCH; ++j) acc[j] = 0.0;

  for (unsigned t = 0; t < tiles_per_wave; ++t)
  {
    DnaTile w;
    if (!dna_tile(w, blockIdx.x, tiles_per_wave, t, e.sites)) break;
    const unsigned n = w.n;
    double va[4][4], vb[4][4], v[4][4];
    if (c.ltip) // wave-uniform
      dna_tip_rows(va, c.ltip[n]);
    else
    {
#pragma unroll
      for (int k = 0; k < 4; ++k) dna_fetch<false>(va[k], c.left + w.off, k, 0u);
    }
    if (c.rtip)
      dna_tip_rows(vb, c.rtip[n]);
    else
    {
#pragma unroll
      for (int k = 0; k < 4; ++k) dna_fetch<false>(vb[k], c.right + w.off, k, 0u);
    }
    unsigned code[QCH];
#pragma unroll
    for (int j = 0; j < QCH; ++j) code[j] = row[j][n];
    const uint4 sca = dna_load_scaler(c.ltip ? nullptr : c.lscaler, n, scale_mode);
    const uint4 scb = dna_load_scaler(c.rtip ? nullptr : c.rscaler, n, scale_mode);
    const uint4 scs = dna_load_scaler(nullptr, n, scale_mode);
    const int inv = e.invariant ? e.invariant[n] : -1;

    uint4 sc;
    int mode;
    dna_combine(op, scale_mode, va, sca, vb, scb, v, sc, mode);

    unsigned rs[4];
    const unsigned scal = dna_site_scalers(e, sc, scs, rs);
#pragma unroll
    for (int j = 0; j < QCH; ++j)
    {
      if ((unsigned)j >= nqh) continue; // (workgroup-uniform: a chunk that is not full pays for its own queries only)
      double terma = 0.0, terminv = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k)
      {
        double xc[4], tb[4];
        dna_fetch<true>(xc, nullptr, k, code[j]);
        dna_matvec(tb, pm + k * 16, xc);
        dna_site_add(e, k, dna_rate_term(v[k], as_const(e.freqs) + (size_t)e.fidx[k] * 4, tb), rs, scal, inv, terma, terminv);
      }
      if (w.valid) acc[j] += dna_site_finish(e, n, terma, terminv, scal, 0);
    }
  }
#pragma unroll
  for (int j = 0; j < QCH; ++j) acc[j] = wave_sum(acc[j]);
  plc_publish_chunk<QCH>(e, q0, nqh, res_stride, acc, 4u);
}

// ------------------------------------------------------------------------------------------------
// Every other shape: the inserted node as k_insertion_tiled forms it (kernels_generic.h: node_first_pass into the LDS tile,
// the flags, one barrier, node_site_scalings); pass 2 once per query of the chunk over the same tile. (rescale ? v 2^256 : v) pi
// is formed once per value and meets every query's (P x)_i in rate_term_add's order of states. keep == 0 (the tile
// does not fit beside the per-query words) forms the products again in pass 2, once per chunk.
// What belongs to one query of the chunk - the lane's state mask, the wave's running rate term, its two site sums, wave
// 0's sum over the tiles - lives in LDS (7 KB per query) and the loops over the chunk are not unrolled: the registers
// are k_insertion_tiled's, whatever QCH is. A value passes through LDS unchanged, so the rounding sequence of a pair
// is the same.
template <int ICH, int QCH>
__global__ __launch_bounds__(256) void k_placement_tiled(const DevEdge e, const InsCand *cands, const unsigned char *const *qrows, unsigned nq,
                                                         unsigned res_stride, const GenGeo g, const unsigned long long *__restrict__ tipmap,
                                                         unsigned tiles_per_block, unsigned keep)
{
  __shared__ unsigned char flags[kMaxRates][64];
  __shared__ double part[QCH][2][4][64];        // [query][terma, terminv][wave][lane]
  __shared__ double rate_term[QCH][4][64];      // [query][wave][lane]: tr of the rate the wave is at
  __shared__ unsigned long long qmask[QCH][64]; // [query][lane]
  __shared__ double qacc[QCH][64];              // [query][lane], wave 0 only
  extern __shared__ double node[];              // keep: [rate][state][lane]
  const InsCand c = ins_get(cands, blockIdx.y);
  const unsigned lane = gen_lane(), wave = gen_wave();
  const unsigned nw = blockDim.x >> 6;
  const bool ltip = c.ltip != nullptr, rtip = c.rtip != nullptr; // wave-uniform
  const unsigned *lsc = ltip ? nullptr : c.lscaler, *rsc = rtip ? nullptr : c.rscaler, *ssc = nullptr; // a tip end has no scaler
  const unsigned q0 = blockIdx.z * QCH;
  const unsigned nqh = min((unsigned)QCH, nq - q0); // queries of this chunk (workgroup-uniform)
  if (wave == 0)
    for (unsigned j = 0; j < nqh; ++j) qacc[j][lane] = 0.0;

  for (unsigned t = 0; t < tiles_per_block; ++t)
  {
    if (!gen_has_tile(tiles_per_block, t, e.sites)) break;
    const GenTile w = gen_tile(tiles_per_block, t, e.sites);
    const unsigned nn = w.nn;
    // the two ends of the candidate, whose product is the inserted node
    const unsigned long long lmask = ltip ? tip_mask(tipmap, c.ltip[nn]) : 0ull;
    const unsigned long long rmask = rtip ? tip_mask(tipmap, c.rtip[nn]) : 0ull;
    for (unsigned j = wave; j < nqh; j += nw) qmask[j][lane] = tip_mask(tipmap, plc_row(qrows, q0 + j)[nn]); // read after the barrier
    const GenEnd le = gen_end(c.lmat, ltip, c.left, nn, g, lmask), re = gen_end(c.rmat, rtip, c.right, nn, g, rmask);

    for (unsigned k = wave; k < g.R; k += nw) flags[k][lane] = node_first_pass<ICH>(le, re, k, g, node, keep, lane) ? 1 : 0;
    __syncthreads(); // every rate's flag, every query's mask, and the values the wave itself parked

    // the site's scaling count: the children's and the inserted node's own decision
    bool site_small;
    const unsigned scal = node_site_scalings(e.per_rate, lsc, rsc, ssc, nn, g.R, flags, lane, site_small);

    for (unsigned j = 0; j < nqh; ++j) part[j][0][wave][lane] = part[j][1][wave][lane] = 0.0; // terma, terminv
    for (unsigned k = wave; k < g.R; k += nw)
    {
      const bool rescale = e.per_rate ? flags[k][lane] != 0 : site_small;
      const unsigned fi = e.fidx[k];
      for (unsigned j = 0; j < nqh; ++j) rate_term[j][wave][lane] = 0.0;
      for (unsigned ch = 0; ch < g.nchunks; ++ch)
      {
        double v[ICH];
        parked_or_product<ICH>(v, le, re, k, ch, g, node, keep, lane);
        // rate_term_add's a_i pi_i of a node, in place: formed once for every query of the chunk, then its fma per query
        cdouble_p pi = as_const(e.freqs) + (size_t)fi * g.SP + ch * ICH;
#pragma unroll
        for (int i = 0; i < ICH; ++i)
          if (ch * ICH + i < g.S) v[i] = (rescale ? v[i] * PLLGPU_SCALE_FACTOR : v[i]) * pi[i];
#pragma unroll 1
        for (unsigned j = 0; j < nqh; ++j)
        {
          double B[ICH];
          contract<ICH, true>(B, e.mat, k, ch, g, nullptr, qmask[j][lane]);
          double tr = rate_term[j][wave][lane];
#pragma unroll
          for (int i = 0; i < ICH; ++i)
            if (ch * ICH + i < g.S) tr = fma(v[i], B[i], tr);
          rate_term[j][wave][lane] = tr;
        }
      }
#pragma unroll 1
      for (unsigned j = 0; j < nqh; ++j)
      {
        double tr = rate_term[j][wave][lane], terma = part[j][0][wave][lane], terminv = part[j][1][wave][lane];
        if (e.per_rate) tr = rate_scaled(tr, node_rate_scalings(lsc, rsc, ssc, nn, g.R, k, flags, lane), scal);
        edge_rate_add(e, g, k, tr, nn, terma, terminv);
        part[j][0][wave][lane] = terma;
        part[j][1][wave][lane] = terminv;
      }
    }
    __syncthreads();
    if (wave == 0 && w.valid)
    {
#pragma unroll 1
      for (unsigned j = 0; j < nqh; ++j)
      {
        double s[2]; // terma, terminv
        wave_order_sums(s, &part[j][0][0][lane], nw);
        double acc = qacc[j][lane];
        acc += finish_site(s[0], s[1], scal, 0) * (double)e.pattern_weights[w.n];
        qacc[j][lane] = acc;
      }
    }
    __syncthreads(); // flags[], part[], qmask[] and node[] are reused by the next tile
  }
  // only wave 0 holds a sum
  double sums[QCH];
#pragma unroll
  for (int j = 0; j < QCH; ++j) sums[j] = (wave == 0 && (unsigned)j < nqh) ? wave_sum(qacc[j][lane]) : 0.0;
  plc_publish_chunk<QCH>(e, q0, nqh, res_stride, sums, 1u);
}
