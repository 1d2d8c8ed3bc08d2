// kernels_quartet.h - batched NNI scores (pll_gpu_quartet_loglikelihoods).
//
// "What is the log-likelihood if the four subtrees e0..e3 around this inner edge are paired ((e0,e1),(e2,e3)),
// ((e0,e2),(e1,e3)) or ((e0,e3),(e1,e2))?" - asked for every quartet of a list in ONE launch. Per value the reference runs
// pll_update_partials with two ops into two spare nodes (src/partials.c:237-291, scaling rule src/core_partials.c:729-763)
// and pll_compute_edge_loglikelihood between them (src/likelihood.c:586-636). Here both nodes and their scaling decisions
// exist in registers (4 x 4) or LDS (every other shape) only, the four ends are read once for all three arrangements, and
// nothing is written but three partial sums per workgroup; the last workgroup of each value adds that value's partials in
// index order (publish_quartet_sums below: a ticket and a slot row per value).
//
// Grid: x = the site tiles exactly as launch_insertions cuts them (a function of the site count alone), y = the
// quartet. The model travels in a DevEdge (mat, parent, child and the scalers unused; block_sums / counter / result = the
// slots [arrangement][quartet of the launch][workgroup], a ticket per value, the results [arrangement][quartet of the call]);
// the ends of quartet y are quartets[y], read through the scalar path. The pair that holds e0 is the edge's parent end and
// the inner matrix is applied on the other pair, after that pair's rescaling.
// Whether an end is a tip is a wave-uniform branch, as in k_insertion_dna.
#pragma once
#include "kernels_common.h"
#include "kernels_dna.h"
#include "kernels_generic.h"
#include "kernels_placement.h"

struct QEnd // 32 bytes
{
  const double *clv;         // CLV of the end, or null: a tip given by codes
  const unsigned char *tip;  // tip codes or null
  const unsigned *scaler;    // null: the end carries no scaler
  const double *mat;         // PT layout: the end's own branch
};

struct QuartetDesc // 144 bytes
{
  QEnd end[4];
  const double *inner;  // PT layout: the quartet's inner edge
  unsigned tt_rule;     // bit x: end x is a tip the REFERENCE reads with its tip kernels (PLL_ATTRIB_PATTERN_TIP); a pair of
  unsigned pad_;        // two such ends takes no scaling decision (src/core_partials.c:185-186, :65-66)
};
typedef const QuartetDesc __attribute__((address_space(4))) *cquartet_p;

__device__ __forceinline__ QuartetDesc quartet_get(const QuartetDesc *quartets, unsigned y)
{
  cquartet_p p = (cquartet_p)(uintptr_t)quartets + y;
  QuartetDesc r;
#pragma unroll
  for (int x = 0; x < 4; ++x)
  {
    r.end[x].clv = p->end[x].clv;
    r.end[x].tip = p->end[x].tip;
    r.end[x].scaler = p->end[x].scaler;
    r.end[x].mat = p->end[x].mat;
  }
  r.inner = p->inner;
  r.tt_rule = p->tt_rule;
  r.pad_ = 0u;
  return r;
}

// The descriptor of quartet y through the scalar path, as an address the compiler takes as new at every call: what is read
// through it is read where it is used and does not occupy scalar registers from the top of the kernel to its end (the
// 4 x 4 kernel has none to spare: the model, 36 words of descriptor and 32 of matrix coefficients at a time).
__device__ __forceinline__ cquartet_p quartet_at(const QuartetDesc *quartets, unsigned y)
{
  const QuartetDesc *p = quartets + y;
  asm volatile("" : "+s"(p));
  return (cquartet_p)(uintptr_t)p;
}

// the partner of e0 in arrangement a, and the other pair in the order the public header writes it
__device__ __forceinline__ void quartet_pairs(int a, int &y, int &z, int &w)
{
  y = a + 1;
  z = a == 0 ? 2 : 1;
  w = a == 2 ? 2 : 3;
}

// end x of quartet y for a wave-uniform x that is no compile-time constant: read again through the scalar path (indexing
// the copy in registers by x would put it into scratch)
__device__ __forceinline__ QEnd quartet_end(const QuartetDesc *quartets, unsigned y, int x)
{
  cquartet_p p = (cquartet_p)(uintptr_t)quartets + y;
  QEnd r;
  r.clv = p->end[x].clv;
  r.tip = p->end[x].tip;
  r.scaler = p->end[x].scaler;
  r.mat = p->end[x].mat;
  return r;
}

__device__ __forceinline__ bool quartet_pair_decides(unsigned tt_rule, int x, int y)
{
  return ((tt_rule >> x) & (tt_rule >> y) & 1u) == 0u;
}

// The 16 coefficients of one rate of a matrix, not to be asked for before `after` exists. Left alone, the compiler asks for
// all 64 coefficients of a matrix in one burst ahead of the arithmetic - 128 scalar registers at a time, more than there
// are - parks them in lanes of a dozen vector registers this kernel has no room for, and reads them back one by one.
__device__ __forceinline__ cdouble_p coefficients_after(const double *pt_k, double after)
{
  asm volatile("" : "+s"(pt_k) : "v"(after));
  return as_const(pt_k);
}

// Three sums per workgroup, handed off side by side: arrangement a of quartet y is plc_publish_chunk's pair (a, y) - thread a
// serves it, so the three stores, waits and tickets are one round trip to the coherent level, not three (kernels_placement.h
// has the measurement). A value owns gridDim.x slots and a ticket: its bits depend on its own workgroups alone. Results leave
// as [arrangement][quartet of the call], rows res_stride apart; the launcher turns them into [quartet][3].
__device__ __forceinline__ void publish_quartet_sums(const DevEdge &e, unsigned res_stride, const double (&wave_value)[3], unsigned nsum_waves)
{
  plc_publish_chunk<3>(e, 0u, 3u, res_stride, wave_value, nsum_waves);
}

// Where the PS instantiations leave every site's value (pll_gpu_quartet_resampled_loglikelihoods);
// value = 3 * (quartet of the launch) + arrangement. The other instantiations take the argument and never read it.
struct QuartetSites
{
  double *u;        // [value][sites padded to the 64-site tile]: the site's log-likelihood BEFORE its pattern weight, 0.0 in the
                    // padding lanes (kernels_resample.h contracts these rows with the replicates' weights); or null
  double *weighted; // [value][sites]: that times the partition's pattern weight - the reference's persite_lnl; or null
};

// the site's value is final: both forms leave (site n of tile `tile`, a lane past the end: valid false, n clamped). The lane
// is read from threadIdx again: one register fewer across the kernels' peak.
__device__ __forceinline__ void quartet_site_store(const QuartetSites &ps, const DevEdge &e, int a, unsigned tile, unsigned n, bool valid, double u,
                                                   double site)
{
  const size_t value = (size_t)3 * blockIdx.y + a;
  const size_t upad = (size_t)((e.sites + 63u) / 64u) * 64u;
  if (ps.u) ps.u[value * upad + (size_t)tile * 64u + (threadIdx.x & 63u)] = valid ? u : 0.0;
  if (ps.weighted && valid) ps.weighted[value * e.sites + n] = site;
}

// ------------------------------------------------------------------------------------------------
// 4 states x 4 rates: one wave per 64-site tile, the lane owns its site. The four ends are loaded (or decoded) once and
// each end's matrix is applied once: pa[x] = P_x e_x, 4 x 16 values = 128 registers that all three arrangements share.
// Per arrangement both nodes are formed from the elementwise products with the update kernels' own step (dna_join: products,
// scaling decision, rescaling, scaler words), the second is contracted with the inner matrix AFTER its rescaling and the
// site likelihood is mixed with the edge kernels' pieces. Two waves per SIMD (256 registers) and no scratch is the budget
// (DESIGN.md section 5.8 has the report); what it took: the scaling mode at compile time, the per-rate form rate by rate,
// descriptor and coefficients read where they are used, the running sums in LDS.
// PS: every site's value also leaves through `ps` (QuartetSites above), stored where it is final - far from the register peak.
template <int SM, bool PS = false> // the partition's scaling mode (1: per site, 2: per rate), at compile time: the other mode's words cost registers
__global__ __launch_bounds__(256, 2) void k_quartet_dna(const DevEdge e, const QuartetDesc *quartets, unsigned res_stride, unsigned tiles_per_wave,
                                                        const QuartetSites ps)
{
  constexpr int scale_mode = SM;
  // the lane's three running sums wait in LDS, each in a word only its lane touches: across the tile loop they would be six
  // more registers than the per-rate form has (it then spills exactly these)
  __shared__ double acc[3][256];
  acc[0][threadIdx.x] = acc[1][threadIdx.x] = acc[2][threadIdx.x] = 0.0;

  for (unsigned t = 0; t < tiles_per_wave; ++t)
  {
    DnaTile w;
    if (!dna_tile(w, blockIdx.x, tiles_per_wave, t, e.sites)) break;
    const unsigned n = w.n;
    double pa[4][4][4];
    uint4 below = make_uint4(0, 0, 0, 0); // the four ends' counts added up: the same under every arrangement
#pragma unroll
    for (int x = 0; x < 4; ++x)
    {
      cquartet_p d = quartet_at(quartets, blockIdx.y);
      const unsigned char *tip = d->end[x].tip;
      const double *mat = d->end[x].mat;
      double v[4][4];
      uint4 sx = make_uint4(0, 0, 0, 0);
      if (tip) // wave-uniform
        dna_tip_rows(v, tip[n]);
      else
      {
        const double *clv = d->end[x].clv;
#pragma unroll
        for (int k = 0; k < 4; ++k) dna_fetch<false>(v[k], clv + w.off, k, 0u);
        sx = dna_load_scaler(d->end[x].scaler, n, scale_mode);
      }
      below = make_uint4(below.x + sx.x, below.y + sx.y, below.z + sx.z, below.w + sx.w);
#pragma unroll
      for (int k = 0; k < 4; ++k) dna_matvec(pa[x][k], coefficients_after(mat + k * 16, k ? pa[x][k - 1][3] : v[0][0]), v[k]);
    }
    const int inv = e.invariant ? e.invariant[n] : -1;

#pragma unroll
    for (int a = 0; a < 3; ++a)
    {
      int y, z, ww;
      quartet_pairs(a, y, z, ww);
      cquartet_p d = quartet_at(quartets, blockIdx.y);
      const unsigned tt_rule = d->tt_rule;
      const double *inner = d->inner;
      const int mode1 = quartet_pair_decides(tt_rule, 0, y) ? scale_mode : 0, mode2 = quartet_pair_decides(tt_rule, z, ww) ? scale_mode : 0;
      const uint4 none = make_uint4(0, 0, 0, 0);
      // Both nodes of a window of rates (dna_join: products, scaling decision, rescaling, scaler words), then rate by rate the
      // second node through the inner matrix and the rate's term. Per-site scaling decides over all four rates: one window.
      // Per-rate scaling: a window per rate, so that one rate's 24 values are live beside the 128 shared ones, not 64.
      // The ends' counts enter once, with the first node: only the sum of both nodes' words is read, and it is the same.
      constexpr int W = SM == 2 ? 1 : 4;
      uint4 sc1 = below, sc2 = none;
      double tr[4];
#pragma unroll
      for (int k0 = 0; k0 < 4; k0 += W)
      {
        double v1[4][4], v2[4][4];
        uint4 s1, s2;
        if (W == 1)
        {
          if (k0 == 0) dna_join<0, 1>(mode2, pa[z], none, pa[ww], none, v2, s2), dna_join<0, 1>(mode1, pa[0], none, pa[y], none, v1, s1);
          if (k0 == 1) dna_join<1, 2>(mode2, pa[z], none, pa[ww], none, v2, s2), dna_join<1, 2>(mode1, pa[0], none, pa[y], none, v1, s1);
          if (k0 == 2) dna_join<2, 3>(mode2, pa[z], none, pa[ww], none, v2, s2), dna_join<2, 3>(mode1, pa[0], none, pa[y], none, v1, s1);
          if (k0 == 3) dna_join<3, 4>(mode2, pa[z], none, pa[ww], none, v2, s2), dna_join<3, 4>(mode1, pa[0], none, pa[y], none, v1, s1);
        }
        else
        {
          dna_join(mode2, pa[z], none, pa[ww], none, v2, s2);
          dna_join(mode1, pa[0], none, pa[y], none, v1, s1);
        }
        sc1 = make_uint4(sc1.x + s1.x, sc1.y + s1.y, sc1.z + s1.z, sc1.w + s1.w);
        sc2 = make_uint4(sc2.x + s2.x, sc2.y + s2.y, sc2.z + s2.z, sc2.w + s2.w);
#pragma unroll
        for (int k = k0; k < k0 + W; ++k)
        {
          double tb[4];
          dna_matvec(tb, coefficients_after(inner + k * 16, v2[k][3]), v2[k]);
          tr[k] = dna_rate_term(v1[k], as_const(e.freqs) + (size_t)e.fidx[k] * 4, tb);
        }
      }
      unsigned rs[4];
      const unsigned scal = dna_site_scalers(e, sc1, sc2, rs);
      double terma = 0.0, terminv = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k) dna_site_add(e, k, tr[k], rs, scal, inv, terma, terminv);
      if constexpr (PS)
      {
        const double u = finish_site(terma, terminv, scal, 0);
        const double site = u * (double)e.pattern_weights[n];
        quartet_site_store(ps, e, a, w.tile, n, w.valid, u, site);
        if (w.valid) acc[a][threadIdx.x] += site;
      }
      else if (w.valid)
        acc[a][threadIdx.x] += dna_site_finish(e, n, terma, terminv, scal, 0);
    }
  }
  const double sums[3] = {wave_sum(acc[0][threadIdx.x]), wave_sum(acc[1][threadIdx.x]), wave_sum(acc[2][threadIdx.x])};
  publish_quartet_sums(e, res_stride, sums, 4u);
}

// ------------------------------------------------------------------------------------------------
// Every other shape (up to 64 states, any rate count): the tiled kernels' shared pieces (kernels_generic.h: gen_tile,
// node_first_pass, parked_or_product, rate_term_add, wave_order_sums) - workgroup = one tile of one quartet
// at a time, wave w of min(R, 4) owns the rate categories w, w + nw, ... - once per arrangement:
//   pass 1  both nodes' unscaled values A_i B_i of the wave's rates, with the "all below 2^-256" flag per (node, rate, lane);
//   pass 2  after one barrier every rate's flags are known: the site's count is the four ends' counts plus both nodes' own
//           decisions (per-rate scalers: the minimum over the rates, terms brought to it with rate_scaled). Rate by rate the
//           second node is rescaled, contracted with the inner matrix - a lane reads its own column of LDS, stride 64 like a
//           tiled CLV - and dotted with pi_i and the rescaled first node as k_edge_tiled does.
// keep == 1: both nodes stay in LDS from pass 1, node[which][rate][state][lane] (20 x 4: 80 KB). keep == 0 (two tiles do not
// fit): pass 2 forms the products a second time - same arithmetic, same bits - and the second node of the wave's current
// rate passes through a slab of its own, slab[wave][state][lane]. A lane only ever reads LDS values it wrote itself.
// Nothing is shared between the arrangements on these shapes: the four P x of a 20 x 4 tile are 160 KB.
// PS: as k_quartet_dna's.
template <int ICH, bool PS = false>
__global__ __launch_bounds__(256) void k_quartet_tiled(const DevEdge e, const QuartetDesc *quartets, const GenGeo g,
                                                       const unsigned long long *__restrict__ tipmap, unsigned res_stride, unsigned tiles_per_block,
                                                       unsigned keep, const QuartetSites ps)
{
  __shared__ unsigned char flags[2][kMaxRates][64];
  __shared__ double part[2][4][64];
  extern __shared__ double node[]; // keep: [2][rate][state][lane]; else [wave][state][lane]
  const QuartetDesc q = quartet_get(quartets, blockIdx.y);
  const unsigned lane = gen_lane(), wave = gen_wave();
  const unsigned nw = blockDim.x >> 6;
  const size_t node_sz = (size_t)g.R * g.S * 64u;
  double acc[3] = {0.0, 0.0, 0.0};

  for (unsigned t = 0; t < tiles_per_block; ++t)
  {
    if (!gen_has_tile(tiles_per_block, t, e.sites)) break;
    const GenTile w = gen_tile(tiles_per_block, t, e.sites);
    const unsigned tile = w.tile, nn = w.nn;
    const bool valid = w.valid;
    const unsigned long long mask[4] = {q.end[0].tip ? tip_mask(tipmap, q.end[0].tip[nn]) : 0ull, q.end[1].tip ? tip_mask(tipmap, q.end[1].tip[nn]) : 0ull,
                                        q.end[2].tip ? tip_mask(tipmap, q.end[2].tip[nn]) : 0ull, q.end[3].tip ? tip_mask(tipmap, q.end[3].tip[nn]) : 0ull};
    const unsigned *const esc[4] = {q.end[0].tip ? nullptr : q.end[0].scaler, q.end[1].tip ? nullptr : q.end[1].scaler,
                                    q.end[2].tip ? nullptr : q.end[2].scaler, q.end[3].tip ? nullptr : q.end[3].scaler};

#pragma unroll 1
    for (int a = 0; a < 3; ++a)
    {
      int y, z, ww;
      quartet_pairs(a, y, z, ww);
      // the arrangement's two pairs, children in the public header's order (named, not indexed: no register file by index)
      const QEnd a0 = q.end[0], a1 = quartet_end(quartets, blockIdx.y, y), b0 = quartet_end(quartets, blockIdx.y, z), b1 = quartet_end(quartets, blockIdx.y, ww);
      const unsigned long long ma0 = mask[0], ma1 = y == 1 ? mask[1] : y == 2 ? mask[2] : mask[3];
      const unsigned long long mb0 = z == 1 ? mask[1] : mask[2], mb1 = ww == 2 ? mask[2] : mask[3];
      const bool decides1 = quartet_pair_decides(q.tt_rule, 0, y), decides2 = quartet_pair_decides(q.tt_rule, z, ww);

      // the ends as the contraction reads them: the first node is above ea0 and ea1, the second above eb0 and eb1
      const GenEnd ea0 = gen_end(a0.mat, a0.tip != nullptr, a0.clv, nn, g, ma0), ea1 = gen_end(a1.mat, a1.tip != nullptr, a1.clv, nn, g, ma1);
      const GenEnd eb0 = gen_end(b0.mat, b0.tip != nullptr, b0.clv, nn, g, mb0), eb1 = gen_end(b1.mat, b1.tip != nullptr, b1.clv, nn, g, mb1);
      // the ends' counts of rate k (per-rate scalers) under both nodes
      auto below_rate = [&](unsigned k) __attribute__((always_inline)) {
        return scaler_sum_rate(esc[0], nn, esc[1], nn, g.R, k) + scaler_sum_rate(esc[2], nn, esc[3], nn, g.R, k);
      };

      for (unsigned k = wave; k < g.R; k += nw)
      {
        flags[0][k][lane] = (node_first_pass<ICH>(ea0, ea1, k, g, node, keep, lane) && decides1) ? 1 : 0;
        flags[1][k][lane] = (node_first_pass<ICH>(eb0, eb1, k, g, node + node_sz, keep, lane) && decides2) ? 1 : 0;
      }
      __syncthreads(); // every rate's flags

      bool site_small[2] = {true, true};
      unsigned scal;
      if (e.per_rate)
      {
        scal = 0xFFFFFFFFu;
        for (unsigned k = 0; k < g.R; ++k) scal = min(scal, below_rate(k) + flags[0][k][lane] + flags[1][k][lane]);
      }
      else
      {
        for (unsigned k = 0; k < g.R; ++k)
        {
          site_small[0] = site_small[0] && flags[0][k][lane];
          site_small[1] = site_small[1] && flags[1][k][lane];
        }
        scal = scaler_sum(esc[0], nn, esc[1], nn) + scaler_sum(esc[2], nn, esc[3], nn) + (site_small[0] ? 1u : 0u) + (site_small[1] ? 1u : 0u);
      }

      double terma = 0.0, terminv = 0.0;
      for (unsigned k = wave; k < g.R; k += nw)
      {
        const bool rescale1 = e.per_rate ? flags[0][k][lane] != 0 : site_small[0];
        const bool rescale2 = e.per_rate ? flags[1][k][lane] != 0 : site_small[1];
        // the second node of rate k, rescaled, where the contraction reads it
        double *second = node + (keep ? node_sz + (size_t)k * g.S * 64u : (size_t)wave * g.S * 64u) + lane;
        for (unsigned ch = 0; ch < g.nchunks; ++ch)
        {
          double v[ICH];
          double *at = second + (size_t)ch * ICH * 64u;
          parked_or_product<ICH>(v, eb0, eb1, k, ch, g, node + node_sz, keep, lane);
          if (keep && !rescale2) continue; // as parked
#pragma unroll
          for (int i = 0; i < ICH; ++i)
            if (ch * ICH + i < g.S) at[(size_t)i * 64] = rescale2 ? v[i] * PLLGPU_SCALE_FACTOR : v[i];
        }
        const unsigned fi = e.fidx[k];
        double tr = 0.0;
        for (unsigned ch = 0; ch < g.nchunks; ++ch)
        {
          double v[ICH], B[ICH];
          parked_or_product<ICH>(v, ea0, ea1, k, ch, g, node, keep, lane);
          contract<ICH, false>(B, q.inner, k, ch, g, second, 0ull);
          tr = rate_term_add<ICH>(tr, v, rescale1, as_const(e.freqs) + (size_t)fi * g.SP + ch * ICH, B, ch, g);
        }
        if (e.per_rate) tr = rate_scaled(tr, below_rate(k) + flags[0][k][lane] + flags[1][k][lane], scal);
        edge_rate_add(e, g, k, tr, nn, terma, terminv);
      }
      part[0][wave][lane] = terma;
      part[1][wave][lane] = terminv;
      __syncthreads();
      if (wave == 0 && (valid || PS))
      {
        double s[2]; // terma, terminv
        wave_order_sums(s, &part[0][0][lane], nw);
        const double u = finish_site(s[0], s[1], scal, 0), pw = (double)e.pattern_weights[nn];
        if constexpr (PS) quartet_site_store(ps, e, a, tile, nn, valid, u, u * pw);
        if (valid)
        {
          // the fused form the compiler gives `acc += u * pw` while nothing else reads the product - written out, so that the
          // instantiation that also stores the product adds the same bits
          if (a == 0) acc[0] = fma(u, pw, acc[0]);
          if (a == 1) acc[1] = fma(u, pw, acc[1]);
          if (a == 2) acc[2] = fma(u, pw, acc[2]);
        }
      }
      __syncthreads(); // flags[], part[] and node[] are reused by the next arrangement / tile
    }
  }
  // only wave 0 holds sums
  const double sums[3] = {wave == 0 ? wave_sum(acc[0]) : 0.0, wave == 0 ? wave_sum(acc[1]) : 0.0, wave == 0 ? wave_sum(acc[2]) : 0.0};
  publish_quartet_sums(e, res_stride, sums, 1u);
}
