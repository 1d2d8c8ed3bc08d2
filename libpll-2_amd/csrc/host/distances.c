/* distances.c - pll_gpu_pairwise_distances (include/pll_amd.h; csrc/hip/kernels_distance.h): the
 * maximum-likelihood distance between every two tips of a list in one device call.
 *
 * Both ends of a pair are tips given by codes, so nothing of a pair is prepared on the host: the call validates, refuses,
 * brings the model, the two contraction matrices of pll_update_sumtable (derivatives.c), the code -> mask map and the code
 * rows of the named tips up to date on the device, and hands the list over. The refusals and the error convention are
 * batch.c's, shared with the other batched calls. */
#include <math.h>

#include "pll_internal.h"

/* codes the device's table has for this partition: what pllgpu_pairwise_distances will count after the flush */
static unsigned int code_count(const pll_partition_t *p, const pll_amd_ext_t *x)
{
  if (p->states == 4) return 16;
  return (p->attributes & PLL_ATTRIB_PATTERN_TIP) ? p->maxstates : (x ? x->ctip_count : 0);
}

/* every check of a list of count > 0 tips behind the one of the outputs, in the order include/pll_amd.h states, the
 * device last; nothing is flushed (shared with pll_gpu_distance_tree, nj.c) */
int pll_distances_check(const char *who, pll_partition_t *p, const unsigned int *tips, unsigned int count, const unsigned int *params_indices,
                        const pll_gpu_newton_t *options, pll_amd_ext_t **ext)
{
  unsigned int i, k;
  if (!tips || !params_indices || !options)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: tips, params_indices or options is NULL", who);
    return pll_batch_fail(who);
  }
  for (i = 0; i < count; ++i)
    if (tips[i] >= p->tips)
    {
      pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: tips[%u] = %u is no tip", who, i, tips[i]);
      return pll_batch_fail(who);
    }
  if (!(options->t_min >= 0) || !(options->t_min <= options->t_max) || !isfinite(options->t_max) || !isfinite(options->t_start) ||
      !(options->tolerance > 0) || options->max_iters < 1 || options->max_iters > PLL_GPU_NEWTON_MAX_ITERS)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: options out of range (t_start %g, bounds [%g, %g], tolerance %g, max_iters %u)", who,
                  options->t_start, options->t_min, options->t_max, options->tolerance, options->max_iters);
    return pll_batch_fail(who);
  }
  if (options->matrix_index != -1)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: matrix_index is %d; a list of pairs leaves no matrix: it must be -1", who, options->matrix_index);
    return pll_batch_fail(who);
  }
  for (k = 0; k < p->rate_cats; ++k)
    if (params_indices[k] >= p->rate_matrices)
    {
      pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: params_indices[%u] out of range", who, k);
      return pll_batch_fail(who);
    }
  for (i = 0; i < count; ++i)
    if (!pll_tip_by_codes(p, tips[i]))
    {
      pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: tip %u (tips[%u]) is not given by codes", who, tips[i], i);
      return pll_batch_fail(who);
    }
  if (!pll_batch_refusals(who, p, "pll_compute_likelihood_derivatives")) return PLL_FAILURE;
  for (k = 0; k < p->rate_cats; ++k)
    if (p->prop_invar[params_indices[k]] > 0)
    {
      /* the invariant term pinv pi[inv] belongs to the alignment column, not to the pair of codes */
      pll_set_error(PLL_ERROR_GPU_UNSUPPORTED, "%s: prop_invar %g of rate matrix %u > 0", who, p->prop_invar[params_indices[k]], params_indices[k]);
      return pll_batch_fail(who);
    }
  const unsigned long nc = code_count(p, pll_ext(p));
  if (nc > PLLGPU_DISTANCE_MAX_CODES || PLLGPU_DISTANCE_LDS_BYTES((unsigned long)p->states, (unsigned long)p->rate_cats, nc) > PLLGPU_DISTANCE_LDS_MAX)
  {
    pll_set_error(PLL_ERROR_GPU_UNSUPPORTED, "%s: %lu tip codes at %u states x %u rate categories: at most %u codes and %lu bytes of LDS per workgroup", who,
                  nc, p->states, p->rate_cats, (unsigned int)PLLGPU_DISTANCE_MAX_CODES, PLLGPU_DISTANCE_LDS_MAX);
    return pll_batch_fail(who);
  }
  unsigned long long wsum = 0;
  for (i = 0; i < p->sites; ++i) wsum += p->pattern_weights[i];
  if (wsum >> 32)
  {
    pll_set_error(PLL_ERROR_GPU_UNSUPPORTED, "%s: the pattern weights add up to %llu; the counts are 32-bit words", who, wsum);
    return pll_batch_fail(who);
  }
  return pll_batch_device(who, p, ext);
}

/* the model, the contraction matrices and the code rows of the tips current on the device; the options in the device
 * layer's form */
int pll_distances_flush(const char *who, pll_partition_t *p, pll_amd_ext_t *x, const unsigned int *tips, unsigned int count,
                        const unsigned int *params_indices, const pll_gpu_newton_t *options, pllgpu_newton_t *device_options)
{
  unsigned int i, k;
  if (count >= 2) /* (one tip is no pair: the device layer sets its diagonal entry and launches nothing) */
  {
    /* the reference reads whatever eigensystem is stored; an invalid one is computed here, as pll_update_sumtable does */
    for (k = 0; k < p->rate_cats; ++k)
      if (!p->eigen_decomp_valid[params_indices[k]] && !pll_update_eigen(p, params_indices[k])) return PLL_FAILURE;
    /* (pll_flush_eigen brings the pattern weights and the code -> mask map along) */
    if (!pll_flush_eigen(p, x) || !pll_flush_aux_matrices(p, x, params_indices)) return pll_batch_fail(who);
    for (i = 0; i < count; ++i)
      if (!pll_flush_clv(p, x, tips[i])) return pll_batch_fail(who);
  }
  device_options->t_start = options->t_start;
  device_options->t_min = options->t_min;
  device_options->t_max = options->t_max;
  device_options->tolerance = options->tolerance;
  device_options->max_iters = options->max_iters;
  device_options->matrix_index = -1;
  return PLL_SUCCESS;
}

int pll_gpu_pairwise_distances(pll_partition_t *p, const unsigned int *tips, unsigned int count, const unsigned int *params_indices,
                               const pll_gpu_newton_t *options, const pll_gpu_distances_t *out)
{
  static const char who[] = "pll_gpu_pairwise_distances";
  if (!p || !out || !out->distance)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: partition, out or out->distance is NULL", who);
    return pll_batch_fail(who);
  }
  if (!count) return PLL_SUCCESS; /* no pair, no entry: nothing of the other arguments is read */
  pll_amd_ext_t *x = NULL;
  pllgpu_newton_t opt;
  if (!pll_distances_check(who, p, tips, count, params_indices, options, &x) ||
      !pll_distances_flush(who, p, x, tips, count, params_indices, options, &opt))
    return PLL_FAILURE;
  const pllgpu_distances_t dev = {out->distance, out->p_distance, out->d_f, out->dd_f, out->status, out->iterations};
  if (pllgpu_pairwise_distances(x->ctx, tips, count, params_indices, &opt, &dev) != 0)
  {
    pll_set_gpu_error(who); /* (prints its own line) */
    return PLL_FAILURE;
  }
  return PLL_SUCCESS;
}
