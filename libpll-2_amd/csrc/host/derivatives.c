/* derivatives.c - pll_update_sumtable / pll_compute_likelihood_derivatives (SURVEY.md section 8
 * row f1; reference: src/derivatives.c:239-418 over src/core_derivatives.c).
 *
 * Case selection as in the reference (:264-321): site repeats on either end -> gather maps;
 * PATTERN_TIP with one tip end -> the tip is read as codes and plays the "left" role (:67-79);
 * tip-tip is refused (:278-286). The table is computed into HBM by the CLV-update kernels with the
 * two contraction matrices
 *     M1[k][j][i] = pi_i * inv_eigenvecs[i][j]      (left end)
 *     M2[k][j][i] = eigenvecs[j][i]                 (right end)
 * per rate category k = params_indices[k]; they are rebuilt and uploaded only when an
 * eigensystem, a frequency vector or params_indices changed. The caller's `sumtable` pointer is a
 * handle to one of PLLGPU_SUMTABLE_SLOTS device tables (allocated on first use; beyond that the least
 * recently used is recycled and its handle remembered: an evaluation on a recycled handle fails
 * loudly instead of reading the caller's never-written buffer). pll_gpu_release_sumtable() gives a
 * table's HBM back.
 */
#include <math.h>

#include "pll_internal.h"

static int fail_loudly(const char *what)
{
  fprintf(stderr, "libpll_amd: %s: [%d] %s\n", what, pll_errno, pll_errmsg);
  return PLL_FAILURE;
}

static int was_evicted(const pll_amd_ext_t *x, const double *key)
{
  int i;
  for (i = 0; i < PLLGPU_SUMTABLE_SLOTS; ++i)
    if (x->sumtable_evicted[i] == key) return 1;
  return 0;
}

static int slot_of(pll_amd_ext_t *x, const double *key, int create)
{
  int i, victim = 0;
  for (i = 0; i < PLLGPU_SUMTABLE_SLOTS; ++i)
    if (x->sumtable_key[i] == key)
    {
      x->sumtable_age[i] = ++x->sumtable_clock;
      return i;
    }
  if (!create) return -1;
  for (i = 0; i < PLLGPU_SUMTABLE_SLOTS; ++i)
  {
    if (!x->sumtable_key[i])
    {
      victim = i;
      break;
    }
    if (x->sumtable_age[i] < x->sumtable_age[victim]) victim = i;
  }
  if (x->sumtable_key[victim])
  {
    x->sumtable_evicted[x->sumtable_evicted_next] = x->sumtable_key[victim];
    x->sumtable_evicted_next = (x->sumtable_evicted_next + 1u) % PLLGPU_SUMTABLE_SLOTS;
  }
  for (i = 0; i < PLLGPU_SUMTABLE_SLOTS; ++i) /* the handle is live again */
    if (x->sumtable_evicted[i] == key) x->sumtable_evicted[i] = NULL;
  x->sumtable_key[victim] = key;
  x->sumtable_age[victim] = ++x->sumtable_clock;
  return victim;
}

/* eigensystems, category rates, prop_invar, frequencies: whatever is stale */
static int flush_deriv_model(pll_partition_t *p, pll_amd_ext_t *x) { return pll_flush_eigen(p, x); }

int pll_flush_aux_matrices(pll_partition_t *p, pll_amd_ext_t *x, const unsigned int *params_indices)
{
  const unsigned int s = p->states, sp = p->states_padded, r = p->rate_cats;
  unsigned int k, i, j;
  int same = (x->aux_version == x->eigen_version) && !x->always_upload;
  for (k = 0; same && k < r; ++k) same = (x->aux_params[k] == params_indices[k]);
  if (same) return PLL_SUCCESS;

  double *m = (double *)calloc((size_t)2 * r * s * sp, sizeof(double));
  if (!m)
  {
    pll_set_error(PLL_ERROR_MEM_ALLOC, "Unable to allocate enough memory.");
    return PLL_FAILURE;
  }
  double *m1 = m, *m2 = m + (size_t)r * s * sp;
  for (k = 0; k < r; ++k)
  {
    const double *ev = p->eigenvecs[params_indices[k]];
    const double *iev = p->inv_eigenvecs[params_indices[k]];
    const double *pi = p->frequencies[params_indices[k]];
    for (j = 0; j < s; ++j)
      for (i = 0; i < s; ++i)
      {
        m1[((size_t)k * s + j) * sp + i] = pi[i] * iev[(size_t)i * sp + j];
        m2[((size_t)k * s + j) * sp + i] = ev[(size_t)j * sp + i];
      }
  }
  int rc = pllgpu_aux_matrix_upload(x->ctx, 0, m1) || pllgpu_aux_matrix_upload(x->ctx, 1, m2);
  free(m);
  if (rc)
  {
    pll_set_gpu_error("sumtable matrices upload");
    return PLL_FAILURE;
  }
  x->aux_version = x->eigen_version;
  memcpy(x->aux_params, params_indices, sizeof(unsigned int) * r);
  return PLL_SUCCESS;
}

int pll_update_sumtable(pll_partition_t *p, unsigned int parent_clv_index, unsigned int child_clv_index,
                        int parent_scaler_index, int child_scaler_index,
                        const unsigned int *params_indices, double *sumtable)
{
  pll_amd_ext_t *x = p ? pll_ext(p) : NULL;
  unsigned int k;
  if (!x || !x->ctx)
  {
    pll_set_error(PLL_ERROR_GPU_UNAVAILABLE, "pll_update_sumtable: no MI355X context behind this partition; this library has no CPU path");
    return fail_loudly("pll_update_sumtable");
  }
  if (parent_clv_index >= p->nodes || child_clv_index >= p->nodes || parent_scaler_index >= (int)p->scale_buffers ||
      child_scaler_index >= (int)p->scale_buffers || !sumtable)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "pll_update_sumtable: index out of range");
    return fail_loudly("pll_update_sumtable");
  }
  if (pll_tip_by_codes(p, parent_clv_index) && pll_tip_by_codes(p, child_clv_index))
  {
    if (p->attributes & PLL_ATTRIB_PATTERN_TIP)
    {
      pll_set_error(PLL_ERROR_PARAM_INVALID, "pll_update_sumtable() was called for the tip-tip case!");
      return PLL_FAILURE;
    }
    pll_tip_densify(p, parent_clv_index);
  }
  const int ptip = pll_tip_by_codes(p, parent_clv_index);
  const int ctip = pll_tip_by_codes(p, child_clv_index);
  for (k = 0; k < p->rate_cats; ++k)
  {
    if (params_indices[k] >= p->rate_matrices)
    {
      pll_set_error(PLL_ERROR_PARAM_INVALID, "pll_update_sumtable: params_indices[%u] out of range", k);
      return fail_loudly("pll_update_sumtable");
    }
    /* the reference reads whatever eigensystem is stored; an invalid one is computed here */
    if (!p->eigen_decomp_valid[params_indices[k]] && !pll_update_eigen(p, params_indices[k])) return PLL_FAILURE;
  }
  if (!flush_deriv_model(p, x) || !pll_flush_aux_matrices(p, x, params_indices)) return fail_loudly("pll_update_sumtable");
  if (!pll_flush_clv(p, x, parent_clv_index) || !pll_flush_clv(p, x, child_clv_index) ||
      (!ptip && !pll_flush_scaler(p, x, parent_scaler_index)) || (!ctip && !pll_flush_scaler(p, x, child_scaler_index)) ||
      !pll_flush_repeats(p, x, parent_clv_index) || !pll_flush_repeats(p, x, child_clv_index))
    return fail_loudly("pll_update_sumtable");

  pllgpu_sumtable_t st;
  memset(&st, 0, sizeof st);
  /* a tip given by codes is the left end; otherwise parent left, child right (:142-153) */
  st.left_clv = ctip ? child_clv_index : parent_clv_index;
  st.right_clv = ctip ? parent_clv_index : child_clv_index;
  st.left_scaler = (ptip || ctip) ? PLL_SCALE_BUFFER_NONE : parent_scaler_index;
  st.right_scaler = ctip ? parent_scaler_index : child_scaler_index;
  st.left_is_tip = (ptip || ctip);
  st.gather = pll_repeats_enabled(p) &&
              (p->repeats->pernode_ids[parent_clv_index] || p->repeats->pernode_ids[child_clv_index]);
  const int slot = slot_of(x, sumtable, 1);
  if (pllgpu_update_sumtable(x->ctx, &st, (unsigned)slot) != 0)
  {
    x->sumtable_key[slot] = NULL;
    pll_set_gpu_error("pll_update_sumtable");
    return PLL_FAILURE;
  }
  if (x->eager_mirror && pllgpu_sumtable_download(x->ctx, (unsigned)slot, sumtable) != 0)
  {
    pll_set_gpu_error("pll_update_sumtable (mirror)");
    return PLL_FAILURE;
  }
  return PLL_SUCCESS;
}

int pll_gpu_sync_sumtable(pll_partition_t *p, double *sumtable)
{
  pll_amd_ext_t *x = p ? pll_ext(p) : NULL;
  if (!x || !x->ctx)
  {
    pll_set_error(PLL_ERROR_GPU_UNAVAILABLE, "pll_gpu_sync_sumtable: no MI355X context behind this partition");
    return fail_loudly("pll_gpu_sync_sumtable");
  }
  const int slot = slot_of(x, sumtable, 0);
  if (slot < 0)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "pll_gpu_sync_sumtable: no device table stands for this buffer");
    return PLL_FAILURE;
  }
  if (pllgpu_sumtable_download(x->ctx, (unsigned)slot, sumtable) != 0)
  {
    pll_set_gpu_error("pll_gpu_sync_sumtable");
    return PLL_FAILURE;
  }
  return PLL_SUCCESS;
}

int pll_gpu_release_sumtable(pll_partition_t *p, const double *sumtable)
{
  pll_amd_ext_t *x = p ? pll_ext(p) : NULL;
  int i;
  if (!x || !x->ctx)
  {
    pll_set_error(PLL_ERROR_GPU_UNAVAILABLE, "pll_gpu_release_sumtable: no MI355X context behind this partition");
    return fail_loudly("pll_gpu_release_sumtable");
  }
  for (i = 0; i < PLLGPU_SUMTABLE_SLOTS; ++i)
    if (x->sumtable_evicted[i] == sumtable) x->sumtable_evicted[i] = NULL;
  const int slot = slot_of(x, sumtable, 0);
  if (slot < 0) return PLL_SUCCESS; /* nothing on the device stands for it (any more) */
  x->sumtable_key[slot] = NULL;
  if (pllgpu_sumtable_release(x->ctx, (unsigned)slot) != 0)
  {
    pll_set_gpu_error("pll_gpu_release_sumtable");
    return PLL_FAILURE;
  }
  return PLL_SUCCESS;
}

/* the device slot an evaluation on this handle reads, or -1 with the error set: a recycled handle fails, a table the
 * library has never seen is uploaded */
static int resident_slot(pll_amd_ext_t *x, const double *sumtable, const char *who)
{
  int slot = slot_of(x, sumtable, 0);
  if (slot >= 0) return slot;
  if (was_evicted(x, sumtable))
  {
    pll_set_error(PLL_ERROR_GPU_RUNTIME, "%s: the device table of this sumtable was recycled "
                  "(more than %d live sumtables in one partition); call pll_update_sumtable again", who, PLLGPU_SUMTABLE_SLOTS);
    fail_loudly(who);
    return -1;
  }
  /* a table this library did not produce: the caller's buffer is the truth */
  slot = slot_of(x, sumtable, 1);
  if (pllgpu_sumtable_upload(x->ctx, (unsigned)slot, sumtable) != 0)
  {
    x->sumtable_key[slot] = NULL;
    pll_set_gpu_error(who);
    return -1;
  }
  return slot;
}

int pll_compute_likelihood_derivatives(pll_partition_t *p, int parent_scaler_index, int child_scaler_index,
                                       double branch_length, const unsigned int *params_indices,
                                       const double *sumtable, double *d_f, double *dd_f)
{
  pll_amd_ext_t *x = p ? pll_ext(p) : NULL;
  const int asc_type = (int)(p->attributes & PLL_ATTRIB_AB_MASK);
  if (!x || !x->ctx)
  {
    pll_set_error(PLL_ERROR_GPU_UNAVAILABLE, "pll_compute_likelihood_derivatives: no MI355X context behind this partition; this library has no CPU path");
    return fail_loudly("pll_compute_likelihood_derivatives");
  }
  if (!sumtable || !d_f || !dd_f || !(branch_length >= 0))
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "pll_compute_likelihood_derivatives: invalid argument");
    return fail_loudly("pll_compute_likelihood_derivatives");
  }
  if (!flush_deriv_model(p, x)) return fail_loudly("pll_compute_likelihood_derivatives");
  const int slot = resident_slot(x, sumtable, "pll_compute_likelihood_derivatives");
  if (slot < 0) return PLL_FAILURE;
  /* Stamatakis: the per-state extra entries are ordinary weighted sites (src/core_derivatives.c:733-742) */
  const unsigned int eval_sites = p->sites + (asc_type == PLL_ATTRIB_AB_STAMATAKIS ? p->states : 0);
  if (pllgpu_likelihood_derivatives(x->ctx, (unsigned)slot, branch_length, params_indices, eval_sites, d_f, dd_f) != 0)
  {
    pll_set_gpu_error("pll_compute_likelihood_derivatives");
    return PLL_FAILURE;
  }
  if (asc_type && asc_type != PLL_ATTRIB_AB_STAMATAKIS)
  {
    /* Lewis / Felsenstein (src/core_derivatives.c:851-924): (L, L', L'') of the extra entries with
     * their scaling undone, summed over the states. pattern_weight_sum stands for the reference's
     * on-the-spot sum of pattern_weights[0..sites) (:900-902): equal whenever the weights were set
     * through pll_set_pattern_weights. */
    double lk[3 * 64], asc[3] = {0.0, 0.0, 0.0};
    unsigned int sc[64], n, sum_w_inv = 0;
    if (parent_scaler_index >= (int)p->scale_buffers || child_scaler_index >= (int)p->scale_buffers ||
        !pll_flush_scaler(p, x, parent_scaler_index) || !pll_flush_scaler(p, x, child_scaler_index))
      return fail_loudly("pll_compute_likelihood_derivatives");
    if (pllgpu_asc_derivative_terms(x->ctx, (unsigned)slot, parent_scaler_index, child_scaler_index, params_indices, lk, sc) != 0)
    {
      pll_set_gpu_error("pll_compute_likelihood_derivatives (ascertainment terms)");
      return PLL_FAILURE;
    }
    for (n = 0; n < p->states; ++n)
    {
      const double f = pow(PLL_SCALE_THRESHOLD, (double)sc[n]);
      asc[0] += lk[3 * n + 0] * f;
      asc[1] += lk[3 * n + 1] * f;
      asc[2] += lk[3 * n + 2] * f;
      sum_w_inv += p->pattern_weights[p->sites + n];
    }
    if (asc_type == PLL_ATTRIB_AB_LEWIS)
    {
      const double w = (double)p->pattern_weight_sum;
      *d_f += w * (asc[1] / (asc[0] - 1.0));
      *dd_f += w * (((asc[0] - 1.0) * asc[2] - asc[1] * asc[1]) / ((asc[0] - 1.0) * (asc[0] - 1.0)));
    }
    else if (asc_type == PLL_ATTRIB_AB_FELSENSTEIN)
    {
      *d_f -= sum_w_inv * (asc[1] / asc[0]);
      *dd_f -= sum_w_inv * (((asc[2] * asc[0]) - asc[1] * asc[1]) / (asc[0] * asc[0]));
    }
    else
    {
      pll_set_error(PLL_ERROR_AB_INVALIDMETHOD, "Illegal ascertainment bias algorithm");
      return PLL_FAILURE;
    }
  }
  return PLL_SUCCESS;
}

/* Newton's iteration for one branch length, on the device (include/pll_amd.h; kernels_deriv.h: k_derivatives_newton) */
int pll_gpu_optimize_branch_length(pll_partition_t *p, int parent_scaler_index, int child_scaler_index,
                                   const unsigned int *params_indices, const double *sumtable,
                                   const pll_gpu_newton_t *options, pll_gpu_newton_result_t *result, double *trace)
{
  static const char who[] = "pll_gpu_optimize_branch_length";
  unsigned int k;
  (void)parent_scaler_index; /* the scalers enter through the Lewis / Felsenstein terms alone, which are refused */
  (void)child_scaler_index;
  if (!p)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: NULL partition", who);
    return fail_loudly(who);
  }
  pll_amd_ext_t *x = pll_ext(p);
  if (!x || !x->ctx)
  {
    pll_set_error(PLL_ERROR_GPU_UNAVAILABLE, "%s: no MI355X context behind this partition; this library has no CPU path", who);
    return fail_loudly(who);
  }
  if (!params_indices || !sumtable || !options || !result)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: NULL argument", who);
    return fail_loudly(who);
  }
  if (!(options->t_min >= 0) || !(options->t_min <= options->t_max) || !isfinite(options->t_max) || !isfinite(options->t_start) ||
      !(options->tolerance > 0) || options->max_iters < 1 || options->max_iters > PLL_GPU_NEWTON_MAX_ITERS ||
      options->matrix_index < -1 || options->matrix_index >= (int)p->prob_matrices)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: options out of range (t_start %g, bounds [%g, %g], tolerance %g, max_iters %u, matrix_index %d)",
                  who, options->t_start, options->t_min, options->t_max, options->tolerance, options->max_iters, options->matrix_index);
    return fail_loudly(who);
  }
  for (k = 0; k < p->rate_cats; ++k)
    if (params_indices[k] >= p->rate_matrices)
    {
      pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: params_indices[%u] out of range", who, k);
      return fail_loudly(who);
    }
  const int asc_type = (int)(p->attributes & PLL_ATTRIB_AB_MASK);
  if (asc_type && asc_type != PLL_ATTRIB_AB_STAMATAKIS)
  {
    pll_set_error(PLL_ERROR_GPU_UNSUPPORTED, "%s: the Lewis / Felsenstein correction is host arithmetic after every evaluation; "
                  "iterate over pll_compute_likelihood_derivatives", who);
    return fail_loudly(who);
  }
  for (k = 0; k < p->rate_cats; ++k)
    if (!p->eigen_decomp_valid[params_indices[k]] && !pll_update_eigen(p, params_indices[k])) return PLL_FAILURE;
  if (!flush_deriv_model(p, x)) return fail_loudly(who);
  const int slot = resident_slot(x, sumtable, who);
  if (slot < 0) return PLL_FAILURE;

  pllgpu_newton_t opt;
  pllgpu_newton_result_t res;
  opt.t_start = options->t_start;
  opt.t_min = options->t_min;
  opt.t_max = options->t_max;
  opt.tolerance = options->tolerance;
  opt.max_iters = options->max_iters;
  opt.matrix_index = options->matrix_index;
  /* Stamatakis: the per-state extra entries are ordinary weighted sites (src/core_derivatives.c:733-742) */
  const unsigned int eval_sites = p->sites + (asc_type == PLL_ATTRIB_AB_STAMATAKIS ? p->states : 0);
  /* (a caller of `trace` gets its rows only once the whole call has succeeded: the device layer writes last) */
  if (pllgpu_optimize_branch_length(x->ctx, (unsigned)slot, params_indices, eval_sites, &opt, &res, trace) != 0)
  {
    pll_set_gpu_error(who);
    return PLL_FAILURE;
  }
  if (options->matrix_index >= 0)
  {
    pll_pmatrix_formed_on_device(p, x, params_indices, (unsigned int)options->matrix_index);
    if (x->eager_mirror && !pll_gpu_sync_pmatrix(p, options->matrix_index)) return PLL_FAILURE;
  }
  result->t = res.t;
  result->d_f = res.d_f;
  result->dd_f = res.dd_f;
  result->iterations = res.iterations;
  result->host_waits = res.host_waits;
  result->status = res.status;
  return PLL_SUCCESS;
}

/* pll_gpu_branch_derivatives (include/pll_amd.h): d_f and dd_f of `count` branches in one call,
 * without a table (csrc/hip/kernels_gradient.h); pll_gpu_branch_category_derivatives and pll_gpu_rate_gradient (section
 * 5.13): the same call keeping each rate category's share and contracting it; pll_gpu_qmatrix_gradient (section 5.14): the
 * outer product where those keep the element-wise one. branch_call is the body of all four:
 * validation of the whole list before anything is flushed or launched, which ends the device reads as tip codes, the
 * flushes (model, the two contraction matrices, every named CLV and scaler once). The refusals, the once-per-call
 * bookkeeping of the flushes and the error convention are batch.c's, shared with the other batched calls. */
typedef struct branch_outputs
{
  double *d_f, *dd_f;                /* every entry */
  double *d_cat, *d_rates, *d_scale; /* the per-category entries; d_rates / d_scale: pll_gpu_rate_gradient */
  int per_category;                  /* 0: pll_gpu_branch_derivatives, whose d_f is mandatory */
  double *d_q, *d_root;              /* pll_gpu_qmatrix_gradient (qmatrix != 0): d_q is mandatory */
  int qmatrix;
} branch_outputs_t;

static int branch_call(const char *who, pll_partition_t *p, const pll_gpu_branch_t *branches, unsigned int count,
                       const unsigned int *params_indices, const branch_outputs_t *out)
{
  unsigned int i, k;
  if (!p)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: partition is NULL", who);
    return pll_batch_fail(who);
  }
  if (!count)
  {
    /* sums over no branch */
    if (out->d_rates)
      for (k = 0; k < p->rate_cats; ++k) out->d_rates[k] = 0.0;
    if (out->d_scale) *out->d_scale = 0.0;
    if (out->d_q) memset(out->d_q, 0, sizeof(double) * p->rate_matrices * p->states * p->states);
    if (out->d_root) memset(out->d_root, 0, sizeof(double) * p->rate_matrices * p->states);
    return PLL_SUCCESS;
  }
  if (out->per_category && !out->d_f && !out->dd_f && !out->d_cat && !out->d_rates && !out->d_scale)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: every output is NULL", who);
    return pll_batch_fail(who);
  }
  if (!branches || !params_indices || (out->qmatrix ? !out->d_q : (!out->per_category && !out->d_f)))
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, out->qmatrix        ? "%s: branches, params_indices or d_q is NULL"
                                           : out->per_category ? "%s: branches or params_indices is NULL"
                                                               : "%s: branches, params_indices or d_f is NULL",
                  who);
    return pll_batch_fail(who);
  }
  for (i = 0; i < count; ++i)
  {
    const pll_gpu_branch_t *b = &branches[i];
    if (b->parent_clv_index >= p->nodes || b->child_clv_index >= p->nodes || b->parent_scaler_index < PLL_SCALE_BUFFER_NONE ||
        b->parent_scaler_index >= (int)p->scale_buffers || b->child_scaler_index < PLL_SCALE_BUFFER_NONE ||
        b->child_scaler_index >= (int)p->scale_buffers)
    {
      pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: branch %u has an index out of range", who, i);
      return pll_batch_fail(who);
    }
    if (!(b->branch_length >= 0) || !isfinite(b->branch_length))
    {
      pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: the length of branch %u is negative or not finite", who, i);
      return pll_batch_fail(who);
    }
  }
  for (k = 0; k < p->rate_cats; ++k)
    if (params_indices[k] >= p->rate_matrices)
    {
      pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: params_indices[%u] out of range", who, k);
      return pll_batch_fail(who);
    }
  for (i = 0; i < count; ++i)
    if (pll_tip_by_codes(p, branches[i].parent_clv_index) && pll_tip_by_codes(p, branches[i].child_clv_index))
    {
      /* pll_update_sumtable makes one of them dense; this call writes nothing */
      pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: both ends of branch %u are tips given by codes", who, i);
      return pll_batch_fail(who);
    }
  pll_amd_ext_t *x = NULL;
  if (!pll_batch_refusals(who, p, "pll_compute_likelihood_derivatives")) return PLL_FAILURE;
  if (out->d_rates)
    for (k = 0; k < p->rate_cats; ++k)
      if (!(p->rates[k] > 0) || !isfinite(p->rates[k]))
      {
        /* t / r is the chain rule; a rate of zero has a finite derivative that it does not give */
        pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: category rate %u is %g; d_rates needs rates that are > 0 and finite", who, k, p->rates[k]);
        return pll_batch_fail(who);
      }
  if (out->d_root)
    for (k = 0; k < p->rate_cats; ++k)
      if (p->prop_invar[params_indices[k]] > 0)
      {
        /* the invariant term pinv pi[inv] of a site depends on pi: a per-state sum over the invariant sites, not formed */
        pll_set_error(PLL_ERROR_GPU_UNSUPPORTED, "%s: the frequency part (d_root / d_freqs) with prop_invar %g of rate matrix %u > 0", who,
                      p->prop_invar[params_indices[k]], params_indices[k]);
        return pll_batch_fail(who);
      }
  if (out->qmatrix && !(p->states == 4 && p->rate_cats == 4) &&
      PLLGPU_QGRADIENT_LDS_BYTES((unsigned long)p->states, (unsigned long)p->rate_cats) > PLLGPU_QGRADIENT_LDS_MAX)
  {
    pll_set_error(PLL_ERROR_GPU_UNSUPPORTED, "%s: %u states x %u rate categories need %lu bytes of LDS per workgroup, more than %lu", who, p->states,
                  p->rate_cats, PLLGPU_QGRADIENT_LDS_BYTES((unsigned long)p->states, (unsigned long)p->rate_cats), PLLGPU_QGRADIENT_LDS_MAX);
    return pll_batch_fail(who);
  }
  if (!pll_batch_device(who, p, &x)) return PLL_FAILURE;

  /* the reference reads whatever eigensystem is stored; an invalid one is computed here, as pll_update_sumtable does */
  for (k = 0; k < p->rate_cats; ++k)
    if (!p->eigen_decomp_valid[params_indices[k]] && !pll_update_eigen(p, params_indices[k])) return PLL_FAILURE;
  if (!flush_deriv_model(p, x) || !pll_flush_aux_matrices(p, x, params_indices)) return pll_batch_fail(who);

  /* every named end current on the device, each index once */
  pll_batch_seen_t seen;
  pllgpu_branch_t *dev = (pllgpu_branch_t *)pll_batch_alloc(who, p, &seen, sizeof(pllgpu_branch_t) * count);
  if (!dev) return PLL_FAILURE;
  int ok = 1;
  for (i = 0; ok && i < count; ++i)
  {
    const pll_gpu_branch_t *b = &branches[i];
    const unsigned int clv[2] = {b->parent_clv_index, b->child_clv_index};
    const int scaler[2] = {b->parent_scaler_index, b->child_scaler_index};
    ok = pll_batch_prepare_once(p, x, &seen, clv[0], scaler[0]) && pll_batch_prepare_once(p, x, &seen, clv[1], scaler[1]);
    dev[i].parent_clv = clv[0];
    dev[i].parent_scaler = scaler[0];
    dev[i].child_clv = clv[1];
    dev[i].child_scaler = scaler[1];
    dev[i].parent_is_tip = pll_tip_by_codes(p, clv[0]) ? 1u : 0u;
    dev[i].child_is_tip = pll_tip_by_codes(p, clv[1]) ? 1u : 0u;
    dev[i].branch_length = b->branch_length;
  }
  pll_batch_seen_free(&seen);
  if (!ok)
  {
    free(dev);
    return pll_batch_fail(who);
  }
  const int rc = out->qmatrix      ? pllgpu_qmatrix_gradient(x->ctx, dev, count, params_indices, out->d_q, out->d_root)
                 : out->per_category ? pllgpu_branch_category_derivatives(x->ctx, dev, count, params_indices, out->d_cat, out->d_f, out->dd_f,
                                                                        out->d_rates, out->d_scale)
                                   : pllgpu_branch_derivatives(x->ctx, dev, count, params_indices, out->d_f, out->dd_f);
  free(dev);
  if (rc != 0)
  {
    pll_set_gpu_error(who); /* (prints its own line) */
    return PLL_FAILURE;
  }
  return PLL_SUCCESS;
}

int pll_gpu_branch_derivatives(pll_partition_t *p, const pll_gpu_branch_t *branches, unsigned int count,
                               const unsigned int *params_indices, double *d_f, double *dd_f)
{
  const branch_outputs_t out = {d_f, dd_f, NULL, NULL, NULL, 0, NULL, NULL, 0};
  return branch_call("pll_gpu_branch_derivatives", p, branches, count, params_indices, &out);
}

int pll_gpu_branch_category_derivatives(pll_partition_t *p, const pll_gpu_branch_t *branches, unsigned int count,
                                        const unsigned int *params_indices, double *d_cat, double *d_f, double *dd_f)
{
  const branch_outputs_t out = {d_f, dd_f, d_cat, NULL, NULL, 1, NULL, NULL, 0};
  return branch_call("pll_gpu_branch_category_derivatives", p, branches, count, params_indices, &out);
}

int pll_gpu_rate_gradient(pll_partition_t *p, const pll_gpu_branch_t *branches, unsigned int count, const unsigned int *params_indices,
                          double *d_rates, double *d_scale, double *d_cat, double *d_f)
{
  const branch_outputs_t out = {d_f, NULL, d_cat, d_rates, d_scale, 1, NULL, NULL, 0};
  return branch_call("pll_gpu_rate_gradient", p, branches, count, params_indices, &out);
}

/* ---- the model gradient (include/pll_amd.h; csrc/hip/kernels_qgradient.h) ---------------- */
int pll_gpu_qmatrix_gradient(pll_partition_t *p, const pll_gpu_branch_t *branches, unsigned int count, const unsigned int *params_indices,
                             double *d_q, double *d_root)
{
  const branch_outputs_t out = {NULL, NULL, NULL, NULL, NULL, 0, d_q, d_root, 1};
  return branch_call("pll_gpu_qmatrix_gradient", p, branches, count, params_indices, &out);
}

/* what the chain rule needs of rate matrix m: every frequency above PLL_EIGEN_MINFREQ (the reference eliminates the other
 * states from the eigensystem) and a positive last exchangeability (everything is relative to it) */
static int chain_rule_ok(const char *who, const pll_partition_t *p, unsigned int m)
{
  const unsigned int s = p->states, np = s * (s - 1) / 2;
  unsigned int i;
  for (i = 0; i < s; ++i)
    if (!(p->frequencies[m][i] > 1e-6 /* PLL_EIGEN_MINFREQ */))
    {
      pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: frequency %u of set %u is %g, not above PLL_EIGEN_MINFREQ", who, i, m, p->frequencies[m][i]);
      return pll_batch_fail(who);
    }
  if (!(p->subst_params[m][np - 1] > 0))
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: the last substitution parameter of set %u is %g, not > 0", who, m, p->subst_params[m][np - 1]);
    return pll_batch_fail(who);
  }
  return PLL_SUCCESS;
}

/* With D_xy = d_q[x][y] - d_q[x][x] (an off-diagonal entry of a moves its row's diagonal the other way), Q = a / mean and
 * E = sum_{x != y} D_xy Q_xy:   dF = (1 / mean) sum_{x != y} D_xy da_xy - (E / mean) dmean.
 *   a_xy = s_xy pi_y, mean = 2 sum_{x<y} s_xy pi_x pi_y:
 *   dF/ds_xy  = (D_xy pi_y + D_yx pi_x - 2 E pi_x pi_y) / mean                         (x < y)
 *   dF/dpi_z  = (sum_{x != z} D_xz s_xz - 2 E sum_{x != z} s_xz pi_x) / mean + d_root[z]
 * and s_p = subst_params[p] / subst_params[last]. O(states^2) in all. */
int pll_gpu_subst_gradient_from_dq(const pll_partition_t *p, unsigned int params_index, const double *d_q_m, const double *d_root_m,
                                   double *d_subst, double *d_freqs)
{
  static const char who[] = "pll_gpu_subst_gradient_from_dq";
  unsigned int x, y, k;
  if (!p || !d_q_m || (!d_subst && !d_freqs))
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: partition or d_q is NULL, or no output is asked for", who);
    return pll_batch_fail(who);
  }
  if (params_index >= p->rate_matrices)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: params_index %u out of range", who, params_index);
    return pll_batch_fail(who);
  }
  if (!chain_rule_ok(who, p, params_index)) return PLL_FAILURE;
  const unsigned int s = p->states, np = s * (s - 1) / 2;
  const double *pi = p->frequencies[params_index], *sub = p->subst_params[params_index];
  const double last = sub[np - 1];
  double *ds = (double *)malloc(sizeof(double) * (np + s));
  if (!ds)
  {
    pll_set_error(PLL_ERROR_MEM_ALLOC, "Unable to allocate enough memory.");
    return pll_batch_fail(who);
  }
  double *col = ds + np; /* per state z: sum_{x != z} D_xz s_xz - 2 E sum_{x != z} s_xz pi_x, built in two passes */
  double mean = 0.0, e_mean = 0.0; /* e_mean = E mean = sum_{x != y} D_xy a_xy / mean */
  for (x = 0, k = 0; x < s; ++x)
    for (y = x + 1; y < s; ++y, ++k)
    {
      const double sxy = sub[k] / last;
      const double dxy = d_q_m[x * s + y] - d_q_m[x * s + x], dyx = d_q_m[y * s + x] - d_q_m[y * s + y];
      mean += 2.0 * sxy * pi[x] * pi[y];
      e_mean += dxy * sxy * pi[y] + dyx * sxy * pi[x];
    }
  const double e = e_mean / mean; /* = E: e_mean carries a, not Q = a / mean */
  for (x = 0; x < s; ++x) col[x] = 0.0;
  for (x = 0, k = 0; x < s; ++x)
    for (y = x + 1; y < s; ++y, ++k)
    {
      const double sxy = sub[k] / last;
      const double dxy = d_q_m[x * s + y] - d_q_m[x * s + x], dyx = d_q_m[y * s + x] - d_q_m[y * s + y];
      ds[k] = (dxy * pi[y] + dyx * pi[x] - 2.0 * e * pi[x] * pi[y]) / mean;
      col[y] += dxy * sxy - 2.0 * e * sxy * pi[x];
      col[x] += dyx * sxy - 2.0 * e * sxy * pi[y];
    }
  if (d_subst)
  {
    /* s_p = subst_params[p] / last for p < last; the last entry moves every other s_p */
    double tail = 0.0;
    for (k = 0; k + 1 < np; ++k)
    {
      d_subst[k] = ds[k] / last;
      tail -= sub[k] * d_subst[k];
    }
    d_subst[np - 1] = tail / last;
  }
  if (d_freqs)
    for (x = 0; x < s; ++x) d_freqs[x] = col[x] / mean + (d_root_m ? d_root_m[x] : 0.0);
  free(ds);
  return PLL_SUCCESS;
}

int pll_gpu_subst_gradient(pll_partition_t *p, const pll_gpu_branch_t *branches, unsigned int count, const unsigned int *params_indices,
                           double *d_subst, double *d_freqs)
{
  static const char who[] = "pll_gpu_subst_gradient";
  unsigned int k, m;
  if (!p)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: partition is NULL", who);
    return pll_batch_fail(who);
  }
  const unsigned int s = p->states, np = s * (s - 1) / 2;
  if (!count)
  {
    /* sums over no branch */
    if (d_subst) memset(d_subst, 0, sizeof(double) * p->rate_matrices * np);
    if (d_freqs) memset(d_freqs, 0, sizeof(double) * p->rate_matrices * s);
    return PLL_SUCCESS;
  }
  if (!d_subst && !d_freqs)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: every output is NULL", who);
    return pll_batch_fail(who);
  }
  /* what the chain rule asks of the used sets, before anything else is looked at (a params_indices that cannot be read
   * for this is reported by the list checks below) */
  if (params_indices)
  {
    int in_range = 1;
    for (k = 0; k < p->rate_cats; ++k) in_range &= (params_indices[k] < p->rate_matrices);
    for (k = 0; in_range && k < p->rate_cats; ++k)
      if (!chain_rule_ok(who, p, params_indices[k])) return PLL_FAILURE;
  }
  double *d_q = (double *)malloc(sizeof(double) * p->rate_matrices * (s * s + s + np + s));
  if (!d_q)
  {
    pll_set_error(PLL_ERROR_MEM_ALLOC, "Unable to allocate enough memory.");
    return pll_batch_fail(who);
  }
  double *d_root = d_q + (size_t)p->rate_matrices * s * s, *sub = d_root + (size_t)p->rate_matrices * s, *fr = sub + (size_t)p->rate_matrices * np;
  const branch_outputs_t out = {NULL, NULL, NULL, NULL, NULL, 0, d_q, d_freqs ? d_root : NULL, 1};
  /* the list checks, the refusals and the device call; then what the chain rule asks of the used sets - everything before
   * the caller's arrays are touched */
  int ok = branch_call(who, p, branches, count, params_indices, &out);
  for (m = 0; ok && m < p->rate_matrices; ++m)
  {
    int used = 0;
    for (k = 0; k < p->rate_cats; ++k) used |= (params_indices[k] == m);
    if (!used)
    {
      memset(sub + (size_t)m * np, 0, sizeof(double) * np);
      memset(fr + (size_t)m * s, 0, sizeof(double) * s);
      continue;
    }
    ok = pll_gpu_subst_gradient_from_dq(p, m, d_q + (size_t)m * s * s, d_freqs ? d_root + (size_t)m * s : NULL, sub + (size_t)m * np, fr + (size_t)m * s);
  }
  if (ok)
  {
    if (d_subst) memcpy(d_subst, sub, sizeof(double) * p->rate_matrices * np);
    if (d_freqs) memcpy(d_freqs, fr, sizeof(double) * p->rate_matrices * s);
  }
  free(d_q);
  return ok ? PLL_SUCCESS : PLL_FAILURE;
}
