// kernels_qgradient.h - the model gradient (pll_gpu_qmatrix_gradient): d(-lnL)/dQ of every rate
// matrix, and the root sum's explicit dependence on the frequencies, from the two ends of every branch of a list.
//
// The branch-gradient kernels (kernels_gradient.h) form, per site n and rate category k, the two eigenbasis vectors of a
// sumtable row,
//     A_i = sum_x pi_x p_x U[x][i]   (the left contraction matrix, m1)      B_j = sum_y U^-1[j][y] c_y   (m2),
// and keep the element-wise product A_j B_j. The log-likelihood is multilinear in the P matrices of the branches, and
// dP/dQ in the eigenbasis is a Hadamard product (the Daleckii-Krein form of the Frechet derivative of exp), so the
// derivative with respect to every entry of Q needs the OUTER product, summed over the sites:
//     H_bk[i][j]   = sum_n pw[n] w_k (1 - pinv_k) f_k(n) A_i(n,k) B_j(n,k) / L_n
//     Phi_bk[i][j] = tau e^{lam_j tau} g((lam_i - lam_j) tau),  g(x) = expm1(x) / x, g(0) = 1,  tau = r_k t_b / (1 - pinv_k)
//     W_m[i][j]    = sum_b sum_{k: m(k) = m} Phi_bk[i][j] H_bk[i][j]
//     d_q[m][x][y] = - sum_ij U^-1[i][x] W_m[i][j] U[y][j]
//     d_root[m][x] = - (1 / pi_x) sum_{k: m(k) = m} sum_ij U^-1[i][x] U[x][j] e^{lam_j tau_0k} H_0k[i][j]    (branch 0 only)
// f_k the per-rate excess factor and L_n the site's lk0, both exactly as k_gradient_* form them. Phi is evaluated as
// tau e^{max(lam_i, lam_j) tau} g(-|lam_i - lam_j| tau) - the same number, symmetric, and no exponent is positive; equal
// and nearly equal eigenvalues (JC69: three equal ones) go through expm1 and never through a divided difference.
//
// Stage 1, grid (B workgroups per branch, branches of the launch): a workgroup walks its tiles, accumulates H of its
// branch for every category, and at the end - once per workgroup, not per site - applies Phi, adds the categories of one
// rate matrix in category order and leaves S x S values per used rate matrix in ITS OWN slot (slots[branch][workgroup]
// [matrix][i][j]) with ordinary stores; when d_root is asked every slot is twice as long and the workgroups of the call's
// branch 0 also leave sum_k e^{lam_j tau} H in the second half. An end given by codes plays the left role (m1) as in
// k_gradient_*: when that end is the CHILD the accumulated matrix is the transpose (pi_x U[x][i] = U^-1[i][x] for the
// symmetrised eigensystems pll_update_eigen computes), and the publish step reads it transposed (BranchDesc::pad_ != 0).
//   4 states x 4 categories (k_qgradient_dna): the lane owns a site, 16 accumulators per category in registers, a wave
//   reduction at the end, the four waves added in wave order.
//   every other shape (k_qgradient_mfma): the waves split the categories and form A and B per site with
//   kernels_generic.h's end_contract over k_gradient_tiled's walk (gen_tile), but park them in LDS ([category][state][site], rows 65
//   doubles apart: the lane-per-site stores and the operand reads below are both free of bank conflicts). Once the
//   site's L is known the contraction over the tile's 64 sites runs on the fp64 matrix pipe: v_mfma_f64_16x16x4_f64,
//   lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15], register t of the result is D[(l >> 4) + 4 t][l & 15]
//   (kernels_resample.h is the precedent). States are padded to a multiple of 16 with rows of zeros; the 16 x 16 blocks
//   (category, block row, block column) are dealt to the four waves round-robin, NACC per wave in registers.
// Stage 2 (k_qgradient_slots and k_qgradient_branches behind every cut, k_qgradient_transform behind the last): the slots
// of a branch added in slot order, the branches in list order into W; then d_q and d_root with the eigenvectors the
// contraction matrices hold.
// No ticket, no atomics: every sum has an order that follows from the shape and the list.
#pragma once
#include "kernels_gradient.h"

constexpr unsigned kQgRow = 65; // doubles between two state rows of the parked operands

struct QGeo
{
  unsigned S, SP, SPT, R;
  unsigned Spad;                  // states rounded up to a multiple of 16 (k_qgradient_mfma)
  unsigned nm;                    // rate matrices that a category uses
  unsigned slot;                  // doubles per workgroup slot: nm S S, twice that with d_root
  unsigned char mslot[kMaxRates]; // category -> the position of its rate matrix among the used ones
  unsigned char kfirst[kMaxRates]; // used rate matrix -> the first category that uses it
};

__device__ __forceinline__ bool qg_swapped(const BranchDesc *branches, unsigned y)
{
  cbranch_p p = (cbranch_p)(uintptr_t)branches + y;
  return p->pad_ != 0.0;
}

__device__ __forceinline__ double qg_phi(double li, double lj, double tau)
{
  const double hi = fmax(li, lj), x = -fabs(li - lj) * tau;
  const double g = x == 0.0 ? 1.0 : expm1(x) / x;
  return tau * exp(hi * tau) * g;
}

// The workgroup's H ([category][ld][ld] in LDS, complete behind a barrier) into its slot: Phi applied, the categories of a
// rate matrix added in category order.
__device__ __forceinline__ void qg_publish(const QGeo &q, const DevDiag &dg, double t, bool swapped, bool root_here, const double *Hs, unsigned ld,
                                           double *__restrict__ slot)
{
  const unsigned SS = q.S * q.S;
  for (unsigned idx = threadIdx.x; idx < q.nm * SS; idx += blockDim.x)
  {
    const unsigned ms = idx / SS, ij = idx % SS, i = ij / q.S, j = ij % q.S;
    const unsigned at = swapped ? j * ld + i : i * ld + j;
    double s = 0.0, r = 0.0;
    for (unsigned k = 0; k < q.R; ++k)
    {
      if (q.mslot[k] != ms) continue;
      const unsigned fi = dg.fidx[k];
      const double tau = dg.rates[k] / (1.0 - dg.prop_invar[fi]) * t;
      const double li = dg.eigenvals[(size_t)fi * dg.SP + i], lj = dg.eigenvals[(size_t)fi * dg.SP + j];
      const double h = Hs[(size_t)k * ld * ld + at];
      s = fma(qg_phi(li, lj, tau), h, s);
      if (root_here) r = fma(exp(lj * tau), h, r);
    }
    slot[idx] = s;
    if (root_here) slot[q.nm * SS + idx] = r;
  }
}

// ------------------------------------------------------------------------------------------------
// 4 states x 4 rates: k_gradient_dna's walk (one wave per 64-site tile, the lane owns its site), keeping both vectors of
// every category until the site's L is known.
__global__ __launch_bounds__(256) void k_qgradient_dna(const DevEdge e, const DevDiag dg, const QGeo q, const BranchDesc *branches, const double *m1,
                                                       const double *m2, double *__restrict__ slots, unsigned tiles_per_wave, unsigned root_first)
{
  __shared__ double ldiag[16 * 4];
  __shared__ double red[4][64];
  __shared__ double Hs[64];
  const BranchDesc b = branch_get(branches, blockIdx.y);
  const bool swapped = qg_swapped(branches, blockIdx.y);
  branch_diag(dg, b.t, ldiag);
  cdouble_p lm = as_const(m1), rm = as_const(m2);
  const int smode = e.per_rate ? 2 : 0; // per-site counts cancel: not read
  const unsigned lane = threadIdx.x & 63u;
  const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  double acc[4][16];
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[k][v] = 0.0;

  for (unsigned t = 0; t < tiles_per_wave; ++t)
  {
    DnaTile w;
    if (!dna_tile(w, blockIdx.x, tiles_per_wave, t, e.sites)) break;
    const unsigned n = w.n;
    const uint4 ls = dna_load_scaler(b.lscaler, n, smode), rs = dna_load_scaler(b.rscaler, n, smode);
    const unsigned sk[4] = {ls.x + rs.x, ls.y + rs.y, ls.z + rs.z, ls.w + rs.w};
    const unsigned mn = min(min(sk[0], sk[1]), min(sk[2], sk[3]));
    const int inv = e.invariant ? e.invariant[n] : -1;
    const unsigned lcode = b.ltip ? b.ltip[n] : 0u, rcode = b.rtip ? b.rtip[n] : 0u; // wave-uniform choices
    double lk0 = 0.0, lk1 = 0.0, lk2 = 0.0;
    double pa[4][4], pb[4][4], gk[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
    {
      double xl[4], xr[4];
      if (b.ltip)
        dna_fetch<true>(xl, nullptr, k, lcode);
      else
        dna_fetch<false>(xl, b.left + w.off, k, 0u);
      if (b.rtip)
        dna_fetch<true>(xr, nullptr, k, rcode);
      else
        dna_fetch<false>(xr, b.right + w.off, k, 0u);
      dna_matvec(pa[k], lm + k * 16, xl);
      dna_matvec(pb[k], rm + k * 16, xr);
      const double f = excess_factor(sk[k], mn);
      double c0 = 0.0;
#pragma unroll
      for (int j = 0; j < 4; ++j) c0 = fma(pa[k][j] * pb[k][j] * f, ldiag[(k * 4 + j) * 4], c0);
      deriv_rate_add(e.freqs, e.prop_invar, e.rate_weights, e.fidx[k], 4u, k, inv, c0, 0.0, 0.0, lk0, lk1, lk2);
      const double pinv = e.prop_invar ? e.prop_invar[e.fidx[k]] : 0.0;
      gk[k] = e.rate_weights[k] * (1.0 - pinv) * f;
    }
    if (w.valid)
    {
      const double base = (double)e.pattern_weights[n] / lk0;
#pragma unroll
      for (int k = 0; k < 4; ++k)
      {
        const double gw = gk[k] * base;
#pragma unroll
        for (int i = 0; i < 4; ++i)
        {
          const double ai = pa[k][i] * gw;
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[k][i * 4 + j] = fma(ai, pb[k][j], acc[k][i * 4 + j]);
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int v = 0; v < 16; ++v)
    {
      const double s = wave_sum(acc[k][v]);
      if (lane == 0) red[wave][k * 16 + v] = s;
    }
  __syncthreads();
  if (threadIdx.x < 64u) Hs[threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
  __syncthreads();
  qg_publish(q, dg, b.t, swapped, root_first && blockIdx.y == 0, Hs, 4u, slots + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * q.slot);
}

// ------------------------------------------------------------------------------------------------
// Every other shape up to 64 states. 256 threads; dynamic LDS (qg_lds_doubles): the branch's diag table [R][S][4], the
// waves' shares of L [4][64], the site weights [R][64], then the parked operands tA and tB, each [R][Spad][kQgRow]; the
// operand region holds H ([R][Spad][Spad]) on the way out.
static constexpr size_t qg_lds_doubles(unsigned S, unsigned R)
{
  const size_t Spad = (S + 15u) / 16u * 16u;
  return (size_t)R * S * 4 + 4 * 64 + (size_t)R * 64 + 2 * (size_t)R * Spad * kQgRow;
}

typedef double __attribute__((ext_vector_type(4))) qg_double4;

template <int ICH, int NACC>
__global__ __launch_bounds__(256) void k_qgradient_mfma(const DevEdge e, const DevDiag dg, const QGeo q, const BranchDesc *branches, const double *m1,
                                                        const double *m2, const GenGeo g, const unsigned long long *__restrict__ tipmap,
                                                        double *__restrict__ slots, unsigned tiles_per_block, unsigned root_first)
{
  extern __shared__ double qlds[];
  const unsigned Spad = q.Spad, nb = Spad >> 4, NB = g.R * nb * nb;
  double *const ldiag = qlds, *const part = ldiag + (size_t)g.R * g.S * 4, *const wgt = part + 256, *const tA = wgt + (size_t)g.R * 64,
                *const tB = tA + (size_t)g.R * Spad * kQgRow;
  const BranchDesc b = branch_get(branches, blockIdx.y);
  const bool swapped = qg_swapped(branches, blockIdx.y);
  // the padding rows (states S .. Spad) stay zero: nothing below writes them
  for (unsigned idx = threadIdx.x; idx < 2u * g.R * Spad * kQgRow; idx += 256u) tA[idx] = 0.0;
  branch_diag(dg, b.t, ldiag); // (ends with a barrier)
  const unsigned lane = gen_lane(), wave = gen_wave();
  const unsigned r16 = lane & 15u, q4 = lane >> 4;
  const bool ltip = b.ltip != nullptr, rtip = b.rtip != nullptr; // wave-uniform
  const unsigned *lsc = e.per_rate ? b.lscaler : nullptr, *rsc = e.per_rate ? b.rscaler : nullptr;
  qg_double4 acc[NACC];
#pragma unroll
  for (int a = 0; a < NACC; ++a) acc[a] = qg_double4{0.0, 0.0, 0.0, 0.0};

  for (unsigned t = 0; t < tiles_per_block; ++t)
  {
    if (!gen_has_tile(tiles_per_block, t, e.sites)) break;
    const GenTile w = gen_tile(tiles_per_block, t, e.sites);
    const unsigned nn = w.nn;
    const bool valid = w.valid;
    const unsigned long long lmask = ltip ? tip_mask(tipmap, b.ltip[nn]) : 0ull;
    const unsigned long long rmask = rtip ? tip_mask(tipmap, b.rtip[nn]) : 0ull;
    const GenEnd le = gen_end(m1, ltip, b.left, nn, g, lmask), re = gen_end(m2, rtip, b.right, nn, g, rmask);
    const unsigned mn = e.per_rate ? scaler_min(lsc, nn, rsc, nn, g.R) : 0u;
    const int inv = e.invariant ? e.invariant[nn] : -1;

    double lk0 = 0.0, lk1 = 0.0, lk2 = 0.0;
    for (unsigned k = wave; k < g.R; k += 4u)
    {
      const double f = e.per_rate ? excess_factor(scaler_sum_rate(lsc, nn, rsc, nn, g.R, k), mn) : 1.0;
      double c0 = 0.0;
      for (unsigned ch = 0; ch < g.nchunks; ++ch)
      {
        double A[ICH], B[ICH];
        end_contract<ICH>(A, le, k, ch, g);
        end_contract<ICH>(B, re, k, ch, g);
        const double *dk = ldiag + ((size_t)k * g.S + ch * ICH) * 4; // wave-uniform addresses: LDS broadcast
        double *oa = tA + ((size_t)k * Spad + ch * ICH) * kQgRow + lane, *ob = tB + ((size_t)k * Spad + ch * ICH) * kQgRow + lane;
#pragma unroll
        for (int i = 0; i < ICH; ++i)
          if (ch * ICH + i < g.S)
          {
            c0 = fma(A[i] * B[i] * f, dk[i * 4], c0);
            oa[i * kQgRow] = A[i];
            ob[i * kQgRow] = B[i];
          }
      }
      deriv_rate_add(e.freqs, e.prop_invar, e.rate_weights, e.fidx[k], g.SP, k, inv, c0, 0.0, 0.0, lk0, lk1, lk2);
      const double pinv = e.prop_invar ? e.prop_invar[e.fidx[k]] : 0.0;
      wgt[k * 64u + lane] = e.rate_weights[k] * (1.0 - pinv) * f;
    }
    part[wave * 64u + lane] = lk0;
    __syncthreads();
    {
      const double L = ((part[lane] + part[64u + lane]) + part[128u + lane]) + part[192u + lane];
      const double scale = valid ? (double)e.pattern_weights[nn] / L : 0.0;
      for (unsigned k = wave; k < g.R; k += 4u) wgt[k * 64u + lane] = valid ? wgt[k * 64u + lane] * scale : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < NACC; ++a)
    {
      const unsigned blk = wave + 4u * (unsigned)a;
      if (blk < NB) // wave-uniform
      {
        const unsigned k = blk / (nb * nb), bi = (blk / nb) % nb, bj = blk % nb;
        const double *pa = tA + ((size_t)k * Spad + bi * 16u + r16) * kQgRow + 16u * q4;
        const double *pb = tB + ((size_t)k * Spad + bj * 16u + r16) * kQgRow + 16u * q4;
        const double *pw = wgt + k * 64u + 16u * q4;
#pragma unroll 4
        for (unsigned s = 0; s < 16u; ++s) acc[a] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[s] * pw[s], pb[s], acc[a], 0, 0, 0);
      }
    }
    __syncthreads(); // the operands and part[] are reused by the next tile
  }
  // H of the workgroup over the operands (every wave is past the last tile's barrier)
  double *const Hs = tA;
#pragma unroll
  for (int a = 0; a < NACC; ++a)
  {
    const unsigned blk = wave + 4u * (unsigned)a;
    if (blk < NB)
    {
      const unsigned k = blk / (nb * nb), bi = (blk / nb) % nb, bj = blk % nb;
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) Hs[((size_t)k * Spad + bi * 16u + q4 + 4u * (unsigned)tt) * Spad + bj * 16u + r16] = acc[a][tt];
    }
  }
  __syncthreads();
  qg_publish(q, dg, b.t, swapped, root_first && blockIdx.y == 0, Hs, Spad, slots + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * q.slot);
}

// ------------------------------------------------------------------------------------------------
// Stage 2a, behind every cut, two launches. k_qgradient_slots, grid (ceil(slot / 256), branches of the launch): value v of
// branch y = its workgroups' slots added in slot order, left in the branch's slot 0 (a thread reads and writes its own
// value only). k_qgradient_branches: W[v] (+)= those sums added in list order; the root half (v >= half) takes the call's
// branch 0 alone, in the first cut. One thread per value in both.
__global__ __launch_bounds__(256) void k_qgradient_slots(double *__restrict__ slots, unsigned slot, unsigned half, unsigned blocks, unsigned root_first)
{
  const unsigned v = blockIdx.x * 256u + threadIdx.x, y = blockIdx.y;
  if (v >= slot) return;
  if (v >= half && !(root_first && y == 0)) return; // nobody wrote it
  double *p = slots + (size_t)y * blocks * slot + v;
  double s = p[0];
  for (unsigned x = 1; x < blocks; ++x) s += p[(size_t)x * slot];
  p[0] = s;
}

__global__ __launch_bounds__(256) void k_qgradient_branches(const double *__restrict__ slots, double *__restrict__ W, unsigned slot, unsigned half,
                                                            unsigned blocks, unsigned nbranches, unsigned first_cut)
{
  const unsigned v = blockIdx.x * 256u + threadIdx.x;
  if (v >= slot) return;
  const bool root = v >= half;
  if (root && !first_cut) return;
  double s = first_cut ? 0.0 : W[v];
  const unsigned nbr = root ? 1u : nbranches;
  for (unsigned y = 0; y < nbr; ++y) s += slots[(size_t)y * blocks * slot + v];
  W[v] = s;
}

// Stage 2b, behind the last cut: workgroup ms transforms W of used rate matrix ms. U[y][j] = m1[k][y][j] / pi_y and
// U^-1[i][x] = m2[k][x][i] in the PT layout (k the first category that uses the matrix).
//   d_q[x][y] = - sum_i U^-1[i][x] (sum_j W[i][j] U[y][j])      d_root[x] = - (1 / pi_x) sum_i U^-1[i][x] (sum_j G[i][j] U[x][j])
__global__ __launch_bounds__(256) void k_qgradient_transform(const double *__restrict__ W, const double *__restrict__ m1, const double *__restrict__ m2,
                                                             const double *__restrict__ freqs, const QGeo q, const DevDiag dg, unsigned want_root,
                                                             double *__restrict__ d_q, double *__restrict__ d_root)
{
  extern __shared__ double T[]; // [S][S]
  const unsigned S = q.S, SS = S * S, ms = blockIdx.x, k = q.kfirst[ms];
  const double *pi = freqs + (size_t)dg.fidx[k] * q.SP;
  const double *u = m1 + (size_t)k * S * q.SPT, *ui = m2 + (size_t)k * S * q.SPT;
  const double *Wm = W + (size_t)ms * SS;
  for (unsigned idx = threadIdx.x; idx < SS; idx += 256u)
  {
    const unsigned i = idx / S, y = idx % S;
    double s = 0.0;
    for (unsigned j = 0; j < S; ++j) s = fma(Wm[i * S + j], u[(size_t)y * q.SPT + j], s);
    T[idx] = s / pi[y];
  }
  __syncthreads();
  for (unsigned idx = threadIdx.x; idx < SS; idx += 256u)
  {
    const unsigned x = idx / S, y = idx % S;
    double s = 0.0;
    for (unsigned i = 0; i < S; ++i) s = fma(ui[(size_t)x * q.SPT + i], T[i * S + y], s);
    d_q[(size_t)ms * SS + idx] = -s;
  }
  if (!want_root) return; // (uniform)
  __syncthreads();
  const double *Gm = W + (size_t)q.nm * SS + (size_t)ms * SS;
  for (unsigned idx = threadIdx.x; idx < SS; idx += 256u) // T[i][x] = sum_j G[i][j] U[x][j]
  {
    const unsigned i = idx / S, x = idx % S;
    double s = 0.0;
    for (unsigned j = 0; j < S; ++j) s = fma(Gm[i * S + j], u[(size_t)x * q.SPT + j], s);
    T[idx] = s / pi[x];
  }
  __syncthreads();
  for (unsigned x = threadIdx.x; x < S; x += 256u)
  {
    double s = 0.0;
    for (unsigned i = 0; i < S; ++i) s = fma(ui[(size_t)x * q.SPT + i], T[i * S + x], s);
    d_root[(size_t)ms * S + x] = -s / pi[x];
  }
}
