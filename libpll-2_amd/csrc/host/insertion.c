/* insertion.c - pll_gpu_insertion_loglikelihoods: the log-likelihood of inserting one subtree into each of `count`
 * candidate edges, in one call.
 *
 * lnl[i] is what the reference returns for pll_update_partials with the single operation {tmp, tmp_scaler, child1 of
 * candidate i, child2 of candidate i} (src/partials.c:237-291) followed by pll_compute_edge_loglikelihood(tmp,
 * tmp_scaler, subtree, ...) (src/likelihood.c:586-636) - but no tmp exists: the inserted node lives in the kernel's
 * registers or LDS (csrc/hip/kernels_insertion.h) and nothing in the partition is written.
 *
 * This file: validation of the whole list before anything is flushed or launched, the refusals, which ends the device
 * reads as tip codes, the flushes (model, every named matrix, every named CLV and scaler once), the error convention.
 * Any of the three ends may be an inner CLV, a PLL_ATTRIB_PATTERN_TIP tip or a compact indicator tip. The inserted
 * node is the edge's parent end and P is applied on the subtree side - the reference's own orientation, so no end is
 * swapped and no tip is given a dense CLV.
 *
 * pll_gpu_placement_loglikelihoods asks the same of many query tips at once, over the same
 * candidates: the same checks, refusals, flushes and descriptors, and a list of query tips in place of the subtree end.
 *
 * The refusals, the once-per-call bookkeeping of the flushes and the error convention are batch.c's, shared with the
 * other batched calls; the list checks and their order are this file's. */
#include "pll_internal.h"

static const char *const who = "pll_gpu_insertion_loglikelihoods";
static const char *const who_placement = "pll_gpu_placement_loglikelihoods";

/* the first candidate with an index out of range, or count */
static unsigned int first_bad_candidate(const pll_partition_t *p, const pll_gpu_insertion_t *candidates, unsigned int count)
{
  unsigned int i;
  for (i = 0; i < count; ++i)
  {
    const pll_gpu_insertion_t *c = &candidates[i];
    if (!pll_batch_end_in_range(p, c->child1_clv_index, c->child1_scaler_index, c->child1_matrix_index) ||
        !pll_batch_end_in_range(p, c->child2_clv_index, c->child2_scaler_index, c->child2_matrix_index))
      break;
  }
  return i;
}

/* [*lo, *hi] widened to every matrix the candidates name */
static void matrix_span(const pll_gpu_insertion_t *candidates, unsigned int count, unsigned int *lo, unsigned int *hi)
{
  unsigned int i, k;
  for (i = 0; i < count; ++i)
  {
    const unsigned int m[2] = {candidates[i].child1_matrix_index, candidates[i].child2_matrix_index};
    for (k = 0; k < 2; ++k)
    {
      if (m[k] < *lo) *lo = m[k];
      if (m[k] > *hi) *hi = m[k];
    }
  }
}

/* both ends of every candidate current on the device, and the candidates as the device layer takes them */
static int prepare_candidates(pll_partition_t *p, pll_amd_ext_t *x, pll_batch_seen_t *seen, const pll_gpu_insertion_t *candidates,
                              unsigned int count, pllgpu_insertion_t *dev)
{
  unsigned int i;
  int ok = 1;
  for (i = 0; ok && i < count; ++i)
  {
    const pll_gpu_insertion_t *c = &candidates[i];
    pllgpu_insertion_t *d = &dev[i];
    ok = pll_batch_prepare_once(p, x, seen, c->child1_clv_index, c->child1_scaler_index) &&
         pll_batch_prepare_once(p, x, seen, c->child2_clv_index, c->child2_scaler_index);
    d->child1_clv = c->child1_clv_index;
    d->child1_scaler = c->child1_scaler_index;
    d->child1_matrix = c->child1_matrix_index;
    d->child1_is_tip = pll_tip_by_codes(p, c->child1_clv_index) ? 1u : 0u;
    d->child2_clv = c->child2_clv_index;
    d->child2_scaler = c->child2_scaler_index;
    d->child2_matrix = c->child2_matrix_index;
    d->child2_is_tip = pll_tip_by_codes(p, c->child2_clv_index) ? 1u : 0u;
  }
  return ok;
}

int pll_gpu_insertion_loglikelihoods(pll_partition_t *p, unsigned int subtree_clv_index, int subtree_scaler_index,
                                     unsigned int subtree_matrix_index, const pll_gpu_insertion_t *candidates, unsigned int count,
                                     const unsigned int *freqs_indices, double *lnl)
{
  unsigned int i, k;
  if (!p)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: partition is NULL", who);
    return pll_batch_fail(who);
  }
  if (!count) return PLL_SUCCESS;
  if (!candidates || !lnl || !freqs_indices)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: candidates, lnl or freqs_indices is NULL", who);
    return pll_batch_fail(who);
  }
  if (!pll_batch_end_in_range(p, subtree_clv_index, subtree_scaler_index, subtree_matrix_index))
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: the subtree end has an index out of range", who);
    return pll_batch_fail(who);
  }
  for (k = 0; k < p->rate_cats; ++k)
    if (freqs_indices[k] >= p->rate_matrices)
    {
      pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: freqs_indices[%u] out of range", who, k);
      return pll_batch_fail(who);
    }
  if ((i = first_bad_candidate(p, candidates, count)) < count)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: candidate %u has an index out of range", who, i);
    return pll_batch_fail(who);
  }
  /* (site repeats: the inserted node has no class map; documented as the next step) */
  pll_amd_ext_t *x = NULL;
  if (!pll_batch_refusals_and_device(who, p, "pll_compute_edge_loglikelihood", &x)) return PLL_FAILURE;

  /* inputs current on the device: the model, every named matrix, every named end once */
  unsigned int lo = subtree_matrix_index, hi = subtree_matrix_index;
  matrix_span(candidates, count, &lo, &hi);
  pll_batch_seen_t seen;
  pllgpu_insertion_t *dev = (pllgpu_insertion_t *)pll_batch_alloc(who, p, &seen, sizeof(pllgpu_insertion_t) * count);
  if (!dev) return PLL_FAILURE;
  int ok = pll_flush_model(p, x) && pll_flush_pmatrix(p, x, lo, hi) &&
           pll_batch_prepare_once(p, x, &seen, subtree_clv_index, subtree_scaler_index) &&
           prepare_candidates(p, x, &seen, candidates, count, dev);
  pll_batch_seen_free(&seen);
  if (!ok)
  {
    free(dev);
    return pll_batch_fail(who);
  }
  const int rc = pllgpu_insertion_loglikelihoods(x->ctx, subtree_clv_index, subtree_scaler_index, subtree_matrix_index,
                                                 pll_tip_by_codes(p, subtree_clv_index) ? 1u : 0u, dev, count, freqs_indices, lnl);
  free(dev);
  if (rc != 0)
  {
    pll_set_gpu_error(who); /* (prints its own line) */
    return PLL_FAILURE;
  }
  return PLL_SUCCESS;
}

int pll_gpu_placement_loglikelihoods(pll_partition_t *p, const unsigned int *query_tip_indices, unsigned int query_count,
                                     unsigned int pendant_matrix_index, const pll_gpu_insertion_t *candidates, unsigned int count,
                                     const unsigned int *freqs_indices, double *lnl)
{
  const char *const name = who_placement;
  unsigned int i, k;
  if (!p)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: partition is NULL", name);
    return pll_batch_fail(name);
  }
  if (!query_count || !count) return PLL_SUCCESS;
  if (!query_tip_indices || !candidates || !lnl || !freqs_indices)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: query_tip_indices, candidates, lnl or freqs_indices is NULL", name);
    return pll_batch_fail(name);
  }
  for (i = 0; i < query_count; ++i)
    if (query_tip_indices[i] >= p->tips)
    {
      pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: query %u: %u is no tip of the partition", name, i, query_tip_indices[i]);
      return pll_batch_fail(name);
    }
  if (pendant_matrix_index >= p->prob_matrices)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: the pendant matrix index is out of range", name);
    return pll_batch_fail(name);
  }
  if ((i = first_bad_candidate(p, candidates, count)) < count)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: candidate %u has an index out of range", name, i);
    return pll_batch_fail(name);
  }
  for (k = 0; k < p->rate_cats; ++k)
    if (freqs_indices[k] >= p->rate_matrices)
    {
      pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: freqs_indices[%u] out of range", name, k);
      return pll_batch_fail(name);
    }
  if (!pll_batch_refusals(name, p, "pll_compute_edge_loglikelihood")) return PLL_FAILURE;
  for (i = 0; i < query_count; ++i)
    if (!pll_tip_by_codes(p, query_tip_indices[i]))
    {
      /* the kernel reads a query as one byte per site */
      pll_set_error(PLL_ERROR_GPU_UNSUPPORTED, "%s: query %u: tip %u is not held as codes; set it again with pll_set_tip_states", name, i,
                    query_tip_indices[i]);
      return pll_batch_fail(name);
    }
  pll_amd_ext_t *x = NULL;
  if (!pll_batch_device(name, p, &x)) return PLL_FAILURE;

  /* inputs current on the device: the model, every named matrix, every named end and every query tip once */
  unsigned int lo = pendant_matrix_index, hi = pendant_matrix_index;
  matrix_span(candidates, count, &lo, &hi);
  pll_batch_seen_t seen;
  pllgpu_insertion_t *dev = (pllgpu_insertion_t *)pll_batch_alloc(name, p, &seen, sizeof(pllgpu_insertion_t) * count);
  if (!dev) return PLL_FAILURE;
  int ok = pll_flush_model(p, x) && pll_flush_pmatrix(p, x, lo, hi);
  for (i = 0; ok && i < query_count; ++i) ok = pll_batch_prepare_once(p, x, &seen, query_tip_indices[i], PLL_SCALE_BUFFER_NONE);
  ok = ok && prepare_candidates(p, x, &seen, candidates, count, dev);
  pll_batch_seen_free(&seen);
  if (!ok)
  {
    free(dev);
    return pll_batch_fail(name);
  }
  const int rc = pllgpu_placement_loglikelihoods(x->ctx, query_tip_indices, query_count, pendant_matrix_index, dev, count, freqs_indices, lnl);
  free(dev);
  if (rc != 0)
  {
    pll_set_gpu_error(name); /* (prints its own line) */
    return PLL_FAILURE;
  }
  return PLL_SUCCESS;
}
