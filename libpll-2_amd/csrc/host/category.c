/* category.c - pll_gpu_edge_category_posteriors and pll_gpu_category_weights_em: the
 * per-category site likelihoods of one edge, which every evaluation kernel mixes away in registers, and what model
 * optimisation makes of them - category posteriors, empirical-Bayes site rates, the EM numerators of the category
 * weights, and EM steps on those weights without a trip to the host (csrc/hip/kernels_category.h).
 *
 * This file: the checks in their stated order, all before anything is flushed, launched or written; the ends oriented
 * exactly as pll_compute_edge_loglikelihood orients them (pll_edge_orient, likelihood.c); the category rates on the
 * device. The refusals and the error convention are batch.c's, shared with the batched calls. Nothing in the partition
 * is written: the EM call's start row is read once and its result goes to the caller. */
#include <math.h>

#include "pll_internal.h"

/* what both calls decide after their NULL checks and before a device is needed: the indices of the edge, freqs_indices,
 * two pattern-tip ends, the refusals, the device. PLL_SUCCESS with the partition's extension in *ext. */
static int check_edge_args(const char *who, pll_partition_t *p, unsigned int parent_clv_index, int parent_scaler_index,
                           unsigned int child_clv_index, int child_scaler_index, unsigned int matrix_index,
                           const unsigned int *freqs_indices, pll_amd_ext_t **ext)
{
  unsigned int k;
  if (!pll_batch_end_in_range(p, parent_clv_index, parent_scaler_index, matrix_index) ||
      !pll_batch_end_in_range(p, child_clv_index, child_scaler_index, matrix_index))
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: index out of range", who);
    return pll_batch_fail(who);
  }
  for (k = 0; k < p->rate_cats; ++k)
    if (freqs_indices[k] >= p->rate_matrices)
    {
      pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: freqs_indices[%u] out of range", who, k);
      return pll_batch_fail(who);
    }
  if ((p->attributes & PLL_ATTRIB_PATTERN_TIP) && pll_tip_by_codes(p, parent_clv_index) && pll_tip_by_codes(p, child_clv_index))
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: both ends are pattern tips", who);
    return pll_batch_fail(who);
  }
  return pll_batch_refusals_and_device(who, p, NULL, ext);
}

int pll_gpu_edge_category_posteriors(pll_partition_t *p, unsigned int parent_clv_index, int parent_scaler_index,
                                     unsigned int child_clv_index, int child_scaler_index, unsigned int matrix_index,
                                     const unsigned int *freqs_indices, double *cat_lnl, double *posterior, double *site_rates,
                                     double *weight_sums, double *lnl)
{
  static const char *const who = "pll_gpu_edge_category_posteriors";
  if (!p)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: partition is NULL", who);
    return pll_batch_fail(who);
  }
  if (!freqs_indices)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: freqs_indices is NULL", who);
    return pll_batch_fail(who);
  }
  if (!cat_lnl && !posterior && !site_rates && !weight_sums && !lnl)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: all five outputs are NULL", who);
    return pll_batch_fail(who);
  }
  pll_amd_ext_t *x = NULL;
  if (!check_edge_args(who, p, parent_clv_index, parent_scaler_index, child_clv_index, child_scaler_index, matrix_index,
                       freqs_indices, &x))
    return PLL_FAILURE;
  pllgpu_edge_t e;
  if (!pll_edge_orient(p, x, parent_clv_index, parent_scaler_index, child_clv_index, child_scaler_index, matrix_index,
                       freqs_indices, &e) ||
      (site_rates && !pll_flush_rates(p, x)))
    return pll_batch_fail(who);
  if (pllgpu_edge_category_posteriors(x->ctx, &e, cat_lnl, posterior, site_rates, weight_sums, lnl) != 0)
  {
    pll_set_gpu_error(who); /* (prints its own line) */
    return PLL_FAILURE;
  }
  return PLL_SUCCESS;
}

int pll_gpu_category_weights_em(pll_partition_t *p, unsigned int parent_clv_index, int parent_scaler_index,
                                unsigned int child_clv_index, int child_scaler_index, unsigned int matrix_index,
                                const unsigned int *freqs_indices, const double *start_weights, unsigned int steps,
                                double *weights_out, double *lnl_out)
{
  static const char *const who = "pll_gpu_category_weights_em";
  unsigned int k;
  if (!p)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: partition is NULL", who);
    return pll_batch_fail(who);
  }
  if (!freqs_indices || !weights_out)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: freqs_indices or weights_out is NULL", who);
    return pll_batch_fail(who);
  }
  if (steps > PLL_GPU_EM_MAX_STEPS)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: %u steps, at most %u", who, steps, (unsigned int)PLL_GPU_EM_MAX_STEPS);
    return pll_batch_fail(who);
  }
  const double *start = start_weights ? start_weights : p->rate_weights;
  double total = 0.0;
  for (k = 0; k < p->rate_cats; ++k)
  {
    if (!(start[k] >= 0.0) || !isfinite(start[k]))
    {
      pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: start weight %u is negative or not finite", who, k);
      return pll_batch_fail(who);
    }
    total += start[k];
  }
  if (!(total > 0.0))
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: the start weights sum to 0", who);
    return pll_batch_fail(who);
  }
  pll_amd_ext_t *x = NULL;
  if (!check_edge_args(who, p, parent_clv_index, parent_scaler_index, child_clv_index, child_scaler_index, matrix_index,
                       freqs_indices, &x))
    return PLL_FAILURE;
  pllgpu_edge_t e;
  if (!pll_edge_orient(p, x, parent_clv_index, parent_scaler_index, child_clv_index, child_scaler_index, matrix_index,
                       freqs_indices, &e))
    return pll_batch_fail(who);
  if (pllgpu_category_weights_em(x->ctx, &e, start, steps, weights_out, lnl_out) != 0)
  {
    pll_set_gpu_error(who); /* (prints its own line) */
    return PLL_FAILURE;
  }
  return PLL_SUCCESS;
}
