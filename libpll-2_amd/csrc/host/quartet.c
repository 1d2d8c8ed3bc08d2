/* quartet.c - pll_gpu_quartet_loglikelihoods: the log-likelihoods of all three pairings of the four subtrees around an
 * inner edge, for `count` quartets in one call: what ranking the NNI neighbourhood of a tree asks.
 * pll_gpu_quartet_resampled_loglikelihoods: the same values per site and summed under resampled site weights (DESIGN.md
 * section 5.10): what the SH-like aLRT and RELL supports of the inner branches ask. Both share every check and flush below.
 * pll_gpu_quartet_rell_loglikelihoods: that call with the replicates' weights drawn on the device from a seed, and
 * pll_gpu_draw_replicate_weights: those rows alone.
 *
 * lnl[3 i + a] is what the reference returns for pll_update_partials with the two operations {tmp1, s1, x, y} and
 * {tmp2, s2, z, w} of arrangement a (src/partials.c:237-291) followed by pll_compute_edge_loglikelihood(tmp1, s1, tmp2,
 * s2, inner_matrix_index, ...) (src/likelihood.c:586-636) - but neither tmp exists: both nodes live in the kernel's
 * registers or LDS (csrc/hip/kernels_quartet.h) and nothing in the partition is written.
 *
 * This file: validation of the whole list before anything is flushed or launched, which ends the device reads as tip
 * codes, the flushes (model, one matrix span, every named CLV and scaler once). The refusals, the once-per-call
 * bookkeeping of the flushes and the error convention are batch.c's, shared with the other batched calls. */
#include "pll_internal.h"

/* Everything a call decides after its NULL checks and before a device is needed, in the stated order: every index of the
 * whole list, freqs_indices, the refusals, the device. PLL_SUCCESS with the partition's extension in *ext. */
static int check_list(const char *who, pll_partition_t *p, const pll_gpu_quartet_t *quartets, unsigned int count,
                      const unsigned int *freqs_indices, pll_amd_ext_t **ext)
{
  unsigned int i, k, e;
  for (i = 0; i < count; ++i)
  {
    const pll_gpu_quartet_t *q = &quartets[i];
    int ok = q->inner_matrix_index < p->prob_matrices;
    for (e = 0; e < 4; ++e) ok = ok && pll_batch_end_in_range(p, q->clv_index[e], q->scaler_index[e], q->matrix_index[e]);
    if (!ok)
    {
      pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: quartet %u has an index out of range", who, i);
      return pll_batch_fail(who);
    }
  }
  for (k = 0; k < p->rate_cats; ++k)
    if (freqs_indices[k] >= p->rate_matrices)
    {
      pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: freqs_indices[%u] out of range", who, k);
      return pll_batch_fail(who);
    }
  return pll_batch_refusals_and_device(who, p, "pll_compute_edge_loglikelihood", ext);
}

/* inputs current on the device: the model, one span over every named matrix, every named end once; the device layer's
 * descriptors of the list in *out (the caller frees them) */
static int flush_list(const char *who, pll_partition_t *p, pll_amd_ext_t *x, const pll_gpu_quartet_t *quartets, unsigned int count,
                      pllgpu_quartet_t **out)
{
  unsigned int i, e;
  unsigned int lo = quartets[0].inner_matrix_index, hi = lo;
  for (i = 0; i < count; ++i)
    for (e = 0; e < 5; ++e)
    {
      const unsigned int m = e < 4 ? quartets[i].matrix_index[e] : quartets[i].inner_matrix_index;
      if (m < lo) lo = m;
      if (m > hi) hi = m;
    }
  pll_batch_seen_t seen;
  pllgpu_quartet_t *dev = (pllgpu_quartet_t *)pll_batch_alloc(who, p, &seen, sizeof(pllgpu_quartet_t) * count);
  if (!dev) return PLL_FAILURE;
  /* a pair of two tips takes no scaling decision where the reference reads both with its tip kernels */
  const unsigned int tip_mark = PLLGPU_QUARTET_TIP_CODES | ((p->attributes & PLL_ATTRIB_PATTERN_TIP) ? PLLGPU_QUARTET_TIP_PATTERN : 0u);
  int ok = pll_flush_model(p, x) && pll_flush_pmatrix(p, x, lo, hi);
  for (i = 0; ok && i < count; ++i)
  {
    const pll_gpu_quartet_t *q = &quartets[i];
    pllgpu_quartet_t *d = &dev[i];
    for (e = 0; ok && e < 4; ++e)
    {
      ok = pll_batch_prepare_once(p, x, &seen, q->clv_index[e], q->scaler_index[e]);
      d->clv[e] = q->clv_index[e];
      d->scaler[e] = q->scaler_index[e];
      d->matrix[e] = q->matrix_index[e];
      d->is_tip[e] = pll_tip_by_codes(p, q->clv_index[e]) ? tip_mark : 0u;
    }
    d->inner_matrix = q->inner_matrix_index;
  }
  pll_batch_seen_free(&seen);
  if (!ok)
  {
    free(dev);
    return pll_batch_fail(who);
  }
  *out = dev;
  return PLL_SUCCESS;
}

int pll_gpu_quartet_loglikelihoods(pll_partition_t *p, const pll_gpu_quartet_t *quartets, unsigned int count,
                                   const unsigned int *freqs_indices, double *lnl)
{
  static const char *const who = "pll_gpu_quartet_loglikelihoods";
  if (!p)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: partition is NULL", who);
    return pll_batch_fail(who);
  }
  if (!count) return PLL_SUCCESS;
  if (!quartets || !lnl || !freqs_indices)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: quartets, lnl or freqs_indices is NULL", who);
    return pll_batch_fail(who);
  }
  pll_amd_ext_t *x = NULL;
  pllgpu_quartet_t *dev = NULL;
  if (!check_list(who, p, quartets, count, freqs_indices, &x) || !flush_list(who, p, x, quartets, count, &dev)) return PLL_FAILURE;
  const int rc = pllgpu_quartet_loglikelihoods(x->ctx, dev, count, freqs_indices, lnl);
  free(dev);
  if (rc != 0)
  {
    pll_set_gpu_error(who); /* (prints its own line) */
    return PLL_FAILURE;
  }
  return PLL_SUCCESS;
}

int pll_gpu_quartet_resampled_loglikelihoods(pll_partition_t *p, const pll_gpu_quartet_t *quartets, unsigned int count,
                                             const unsigned int *freqs_indices, const unsigned int *replicate_weights,
                                             unsigned int replicates, double *lnl, double *resampled, double *persite)
{
  static const char *const who = "pll_gpu_quartet_resampled_loglikelihoods";
  if (!p)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: partition is NULL", who);
    return pll_batch_fail(who);
  }
  if (!count) return PLL_SUCCESS;
  if (!quartets || !freqs_indices)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: quartets or freqs_indices is NULL", who);
    return pll_batch_fail(who);
  }
  if (replicates && (!replicate_weights || !resampled))
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: replicates > 0 and replicate_weights or resampled is NULL", who);
    return pll_batch_fail(who);
  }
  if (!lnl && !resampled && !persite)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: lnl, resampled and persite are all NULL", who);
    return pll_batch_fail(who);
  }
  pll_amd_ext_t *x = NULL;
  pllgpu_quartet_t *dev = NULL;
  if (!check_list(who, p, quartets, count, freqs_indices, &x) || !flush_list(who, p, x, quartets, count, &dev)) return PLL_FAILURE;
  /* (pattern weights travel with the model: pll_flush_model) */
  const int rc = pllgpu_quartet_resampled_loglikelihoods(x->ctx, dev, count, freqs_indices, replicate_weights, replicates, lnl,
                                                         replicates ? resampled : NULL, persite);
  free(dev);
  if (rc != 0)
  {
    pll_set_gpu_error(who); /* (prints its own line) */
    return PLL_FAILURE;
  }
  return PLL_SUCCESS;
}

/* the sum of the pattern weights is known on the device only: its refusal is an argument error like the host's own */
static int fail_device(const char *who, int rc)
{
  if (rc != PLLGPU_EINVAL)
  {
    pll_set_gpu_error(who); /* (prints its own line) */
    return PLL_FAILURE;
  }
  pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: %s", who, pllgpu_last_error());
  return pll_batch_fail(who);
}

int pll_gpu_quartet_rell_loglikelihoods(pll_partition_t *p, const pll_gpu_quartet_t *quartets, unsigned int count,
                                        const unsigned int *freqs_indices, unsigned long long seed, unsigned int replicates, double *lnl,
                                        double *resampled, double *persite, unsigned int *replicate_weights)
{
  static const char *const who = "pll_gpu_quartet_rell_loglikelihoods";
  if (!p)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: partition is NULL", who);
    return pll_batch_fail(who);
  }
  if (!count) return PLL_SUCCESS;
  if (!quartets || !freqs_indices)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: quartets or freqs_indices is NULL", who);
    return pll_batch_fail(who);
  }
  if (replicates && !resampled)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: replicates > 0 and resampled is NULL", who);
    return pll_batch_fail(who);
  }
  if (!lnl && !resampled && !persite)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: lnl, resampled and persite are all NULL", who);
    return pll_batch_fail(who);
  }
  pll_amd_ext_t *x = NULL;
  pllgpu_quartet_t *dev = NULL;
  if (!check_list(who, p, quartets, count, freqs_indices, &x) || !flush_list(who, p, x, quartets, count, &dev)) return PLL_FAILURE;
  /* (pattern weights travel with the model: pll_flush_model - the device forms their prefix sums again after an upload) */
  const int rc = pllgpu_quartet_rell_loglikelihoods(x->ctx, dev, count, freqs_indices, seed, replicates, lnl, replicates ? resampled : NULL,
                                                    persite, replicates ? replicate_weights : NULL);
  free(dev);
  return rc != 0 ? fail_device(who, rc) : PLL_SUCCESS;
}

int pll_gpu_draw_replicate_weights(pll_partition_t *p, unsigned long long seed, unsigned int first_replicate, unsigned int replicates,
                                   unsigned int *weights)
{
  static const char *const who = "pll_gpu_draw_replicate_weights";
  if (!p)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: partition is NULL", who);
    return pll_batch_fail(who);
  }
  if (!replicates) return PLL_SUCCESS;
  if (!weights)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: weights is NULL", who);
    return pll_batch_fail(who);
  }
  /* rows the quartet call could not take are not handed out: its refusals */
  pll_amd_ext_t *x = NULL;
  if (!pll_batch_refusals_and_device(who, p, NULL, &x)) return PLL_FAILURE;
  if (!pll_flush_model(p, x)) return pll_batch_fail(who); /* the device's copy of the pattern weights is the partition's */
  const int rc = pllgpu_replicate_weights_draw(x->ctx, seed, first_replicate, replicates, weights);
  return rc != 0 ? fail_device(who, rc) : PLL_SUCCESS;
}

int pll_gpu_resample_last_times(const pll_partition_t *p, double *ms)
{
  pll_amd_ext_t *x = p ? pll_ext(p) : NULL;
  if (!x || !x->ctx || !ms) return PLL_FAILURE;
  return pllgpu_resample_last_times(x->ctx, ms) == 0 ? PLL_SUCCESS : PLL_FAILURE;
}
