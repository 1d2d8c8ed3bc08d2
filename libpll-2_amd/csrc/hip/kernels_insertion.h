// kernels_insertion.h - batched insertion log-likelihoods (pll_gpu_insertion_loglikelihoods).
//
// "What is the log-likelihood if the subtree s is inserted into edge (a, b)?" - asked for every candidate edge of an
// SPR neighbourhood or a placement in ONE launch. Per candidate the reference runs pll_update_partials with one op
// into a spare node (src/partials.c:237-291, scaling rule src/core_partials.c:729-763) and then
// pll_compute_edge_loglikelihood between that node and the subtree (src/likelihood.c:586-636). Here the inserted
// node's CLV and its scaling decision exist in registers (4 x 4) or LDS (every other shape) only: nothing is written
// but one partial sum per workgroup, and the candidate's last workgroup adds them in index order
// (kernels_common.h: publish_candidate_sum).
//
// Grid: x = the site tiles exactly as the unbatched edge kernels cut them (a function of the site count alone),
// y = the candidate. The subtree end and the model are the same for every candidate and travel in a DevEdge
// (child / ctip / cscaler / mat = the subtree end; block_sums / counter / result = the per-candidate slots, tickets and
// results; parent, pscaler, persite unused); the two ends of candidate y are cands[y], read through the scalar path.
// A tip end is given by its codes, whichever of the three ends it is: the inserted node is the edge's parent end and P
// is applied on the subtree side, the reference's own orientation. Whether an end of the candidate is a tip is a
// wave-uniform branch, not a template parameter: one launch serves a list of mixed kinds (register report in DESIGN).
#pragma once
#include "kernels_common.h"
#include "kernels_dna.h"
#include "kernels_generic.h"

struct InsCand // 64 bytes
{
  const double *left, *right;        // CLV of the end, or null: a tip given by codes
  const unsigned char *ltip, *rtip;  // tip codes or null
  const unsigned *lscaler, *rscaler; // null: the end carries no scaler
  const double *lmat, *rmat;         // PT layout
};
typedef const InsCand __attribute__((address_space(4))) *cinscand_p;

__device__ __forceinline__ InsCand ins_get(const InsCand *cands, unsigned y)
{
  cinscand_p p = (cinscand_p)(uintptr_t)cands + y;
  InsCand r;
  r.left = p->left;
  r.right = p->right;
  r.ltip = p->ltip;
  r.rtip = p->rtip;
  r.lscaler = p->lscaler;
  r.rscaler = p->rscaler;
  r.lmat = p->lmat;
  r.rmat = p->rmat;
  return r;
}

// what dna_combine reads of an op; the inserted node always scales (the reference's spare node has a scaler)
struct InsOp
{
  const double *lmat, *rmat;
  bool pscaler;
};

// ------------------------------------------------------------------------------------------------
// 4 states x 4 rates: one wave per 64-site tile, the lane holds its site's 16 values of both ends, forms the inserted
// node with the update kernels' own step (dna_combine: products, scaling decision, rescaling, scaler words - the
// power of two is applied BEFORE the contraction with the subtree side) and mixes the site likelihood with the edge
// kernels' pieces (dna_rate_term / dna_site_scalers / dna_site_add / dna_site_finish).
template <bool STIP>
__global__ __launch_bounds__(256) void k_insertion_dna(const DevEdge e, const InsCand *cands, int scale_mode, unsigned tiles_per_wave)
{
  const InsCand c = ins_get(cands, blockIdx.y);
  InsOp op;
  op.lmat = c.lmat;
  op.rmat = c.rmat;
  op.pscaler = true;
  cdouble_p pm = as_const(e.mat);
  double acc = 0.0;

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
    const unsigned scode = STIP ? e.ctip[n] : 0u;
    const double *__restrict__ sx = STIP ? nullptr : e.child + w.off;
    const uint4 sca = dna_load_scaler(c.ltip ? nullptr : c.lscaler, n, scale_mode);
    const uint4 scb = dna_load_scaler(c.rtip ? nullptr : c.rscaler, n, scale_mode);
    const uint4 scs = dna_load_scaler(STIP ? nullptr : e.cscaler, n, scale_mode);
    const int inv = e.invariant ? e.invariant[n] : -1;

    uint4 sc;
    int mode;
    dna_combine(op, scale_mode, va, sca, vb, scb, v, sc, mode);

    unsigned rs[4];
    const unsigned scal = dna_site_scalers(e, sc, scs, rs);
    double terma = 0.0, terminv = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
    {
      double xc[4], tb[4];
      dna_fetch<STIP>(xc, sx, k, scode);
      dna_matvec(tb, pm + k * 16, xc);
      dna_site_add(e, k, dna_rate_term(v[k], as_const(e.freqs) + (size_t)e.fidx[k] * 4, tb), rs, scal, inv, terma, terminv);
    }
    if (w.valid) acc += dna_site_finish(e, n, terma, terminv, scal, 0);
  }
  publish_candidate_sum(e.block_sums, e.counter, e.result, blockIdx.y, e.fenced, wave_sum(acc), 4u);
}

// ------------------------------------------------------------------------------------------------
// Every other shape (up to 64 states, any rate count): workgroup = one tile of one candidate at a time, wave w of
// min(R, 4) owns the rate categories w, w + nw, ... as in k_partials_tiled / k_edge_tiled, and the pieces are the tiled
// kernels' shared ones (kernels_generic.h: gen_tile, end_product, node_first_pass, node_site_scalings, parked_or_product,
// wave_order_sums; rate_term_add's loop stands written out in pass 2, see there).
//   pass 1  the inserted node's values A_i B_i of the wave's rates, with the "all below 2^-256" flag per (rate, lane);
//           the values stay in LDS, node[rate][state][lane] - 61 x 4 x 64 x 8 B = 125 KB of the 160 KB at the widest
//           supported shape, one workgroup per CU there - where the scaling decision, which needs every rate of the
//           site, finds all of them after one barrier;
//   pass 2  the decision (per site: all rates; per rate: that rate) is added to the two children's counts, the
//           values are rescaled by 2^256 as they are read back - BEFORE they meet the subtree side - and contracted with
//           pi_i (P_s x_s)_i in rate_term_add's order, k_edge_tiled's.
// A shape whose tile does not fit (keep == 0: R x S > 288) computes the products a second time in pass 2 instead of
// keeping them: same arithmetic, same bits, no LDS.
template <int ICH, bool STIP>
__global__ __launch_bounds__(256) void k_insertion_tiled(const DevEdge e, const InsCand *cands, const GenGeo g,
                                                         const unsigned long long *__restrict__ tipmap, unsigned tiles_per_block, unsigned keep)
{
  __shared__ unsigned char flags[kMaxRates][64];
  __shared__ double part[2][4][64];
  extern __shared__ double node[]; // keep: [rate][state][lane]
  const InsCand c = ins_get(cands, blockIdx.y);
  const unsigned lane = gen_lane(), wave = gen_wave();
  const unsigned nw = blockDim.x >> 6;
  const bool ltip = c.ltip != nullptr, rtip = c.rtip != nullptr; // wave-uniform
  const unsigned *lsc = ltip ? nullptr : c.lscaler, *rsc = rtip ? nullptr : c.rscaler, *ssc = STIP ? nullptr : e.cscaler;
  double acc = 0.0;

  for (unsigned t = 0; t < tiles_per_block; ++t)
  {
    if (!gen_has_tile(tiles_per_block, t, e.sites)) break;
    const GenTile w = gen_tile(tiles_per_block, t, e.sites);
    const unsigned nn = w.nn;
    // the two ends of the candidate, whose product is the inserted node, and the subtree end
    const unsigned long long lmask = ltip ? tip_mask(tipmap, c.ltip[nn]) : 0ull;
    const unsigned long long rmask = rtip ? tip_mask(tipmap, c.rtip[nn]) : 0ull;
    const unsigned long long smask = STIP ? tip_mask(tipmap, e.ctip[nn]) : 0ull;
    const GenEnd le = gen_end(c.lmat, ltip, c.left, nn, g, lmask), re = gen_end(c.rmat, rtip, c.right, nn, g, rmask), se = gen_end(e.mat, STIP, e.child, nn, g, smask);

    for (unsigned k = wave; k < g.R; k += nw) flags[k][lane] = node_first_pass<ICH>(le, re, k, g, node, keep, lane) ? 1 : 0;
    __syncthreads(); // every rate's flag, and the values the wave itself parked

    // the site's scaling count: the children's, the inserted node's own decision, the subtree end's
    bool site_small;
    const unsigned scal = node_site_scalings(e.per_rate, lsc, rsc, ssc, nn, g.R, flags, lane, site_small);

    double terma = 0.0, terminv = 0.0;
    for (unsigned k = wave; k < g.R; k += nw)
    {
      const bool rescale = e.per_rate ? flags[k][lane] != 0 : site_small;
      const unsigned fi = e.fidx[k];
      double tr = 0.0;
      for (unsigned ch = 0; ch < g.nchunks; ++ch)
      {
        double v[ICH], B[ICH];
        parked_or_product<ICH>(v, le, re, k, ch, g, node, keep, lane);
        end_contract<ICH>(B, se, k, ch, g);
        // rate_term_add's node form, written out: through the call the 20-state inner instantiation needs 170 registers, two
        // more than the 168 at which three waves share a SIMD
        cdouble_p pi = as_const(e.freqs) + (size_t)fi * g.SP + ch * ICH;
#pragma unroll
        for (int i = 0; i < ICH; ++i)
          if (ch * ICH + i < g.S) tr = fma((rescale ? v[i] * PLLGPU_SCALE_FACTOR : v[i]) * pi[i], B[i], tr);
      }
      if (e.per_rate) tr = rate_scaled(tr, node_rate_scalings(lsc, rsc, ssc, nn, g.R, k, flags, lane), scal);
      edge_rate_add(e, g, k, tr, nn, terma, terminv);
    }
    part[0][wave][lane] = terma;
    part[1][wave][lane] = terminv;
    __syncthreads();
    if (wave == 0 && w.valid)
    {
      double s[2]; // terma, terminv
      wave_order_sums(s, &part[0][0][lane], nw);
      acc += finish_site(s[0], s[1], scal, 0) * (double)e.pattern_weights[w.n];
    }
    __syncthreads(); // flags[], part[] and node[] are reused by the next tile
  }
  // only wave 0 holds a sum
  publish_candidate_sum(e.block_sums, e.counter, e.result, blockIdx.y, e.fenced, wave == 0 ? wave_sum(acc) : 0.0, 1u);
}
