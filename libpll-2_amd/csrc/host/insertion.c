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
 * candidates: the same checks, refusals, flushes and descriptors, and a list of query tips in place of the subtree end. */
#include "pll_internal.h"

static const char *const who = "pll_gpu_insertion_loglikelihoods";
static const char *const who_placement = "pll_gpu_placement_loglikelihoods";

static int fail_as(const char *name)
{
  fprintf(stderr, "libpll_amd: %s: [%d] %s\n", name, pll_errno, pll_errmsg);
  return PLL_FAILURE;
}

static int fail_insertion(void) { return fail_as(who); }

static int end_in_range(const pll_partition_t *p, unsigned int clv, int scaler, unsigned int matrix)
{
  return clv < p->nodes && matrix < p->prob_matrices && scaler >= PLL_SCALE_BUFFER_NONE && scaler < (int)p->scale_buffers;
}

/* the CLV (or tip codes) and scaler of one end on the device, each index once per call */
static int prepare_once(pll_partition_t *p, pll_amd_ext_t *x, unsigned char *seen_clv, unsigned char *seen_scaler, unsigned int clv, int scaler)
{
  const int fresh_clv = !seen_clv[clv];
  const int fresh_scaler = scaler >= 0 && !pll_tip_by_codes(p, clv) && !seen_scaler[scaler];
  if (!fresh_clv && !fresh_scaler) return 1;
  seen_clv[clv] = 1;
  if (scaler >= 0 && !pll_tip_by_codes(p, clv)) seen_scaler[scaler] = 1;
  return pll_prepare_end(p, x, clv, scaler);
}

/* the first candidate with an index out of range, or count */
static unsigned int first_bad_candidate(const pll_partition_t *p, const pll_gpu_insertion_t *candidates, unsigned int count)
{
  unsigned int i;
  for (i = 0; i < count; ++i)
  {
    const pll_gpu_insertion_t *c = &candidates[i];
    if (!end_in_range(p, c->child1_clv_index, c->child1_scaler_index, c->child1_matrix_index) ||
        !end_in_range(p, c->child2_clv_index, c->child2_scaler_index, c->child2_matrix_index))
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
static int prepare_candidates(pll_partition_t *p, pll_amd_ext_t *x, unsigned char *seen, unsigned char *seen_scaler,
                              const pll_gpu_insertion_t *candidates, unsigned int count, pllgpu_insertion_t *dev)
{
  unsigned int i;
  int ok = 1;
  for (i = 0; ok && i < count; ++i)
  {
    const pll_gpu_insertion_t *c = &candidates[i];
    pllgpu_insertion_t *d = &dev[i];
    ok = prepare_once(p, x, seen, seen_scaler, c->child1_clv_index, c->child1_scaler_index) &&
         prepare_once(p, x, seen, seen_scaler, c->child2_clv_index, c->child2_scaler_index);
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
    return fail_insertion();
  }
  if (!count) return PLL_SUCCESS;
  if (!candidates || !lnl || !freqs_indices)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: candidates, lnl or freqs_indices is NULL", who);
    return fail_insertion();
  }
  if (!end_in_range(p, subtree_clv_index, subtree_scaler_index, subtree_matrix_index))
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: the subtree end has an index out of range", who);
    return fail_insertion();
  }
  for (k = 0; k < p->rate_cats; ++k)
    if (freqs_indices[k] >= p->rate_matrices)
    {
      pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: freqs_indices[%u] out of range", who, k);
      return fail_insertion();
    }
  if ((i = first_bad_candidate(p, candidates, count)) < count)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: candidate %u has an index out of range", who, i);
    return fail_insertion();
  }
  if (pll_repeats_enabled(p))
  {
    /* the inserted node has no class map; documented as the next step */
    pll_set_error(PLL_ERROR_GPU_UNSUPPORTED, "%s: PLL_ATTRIB_SITE_REPEATS partitions are not supported", who);
    return fail_insertion();
  }
  if (p->attributes & PLL_ATTRIB_AB_MASK)
  {
    pll_set_error(PLL_ERROR_GPU_UNSUPPORTED, "%s: the ascertainment-bias correction needs pll_compute_edge_loglikelihood", who);
    return fail_insertion();
  }
  pll_amd_ext_t *x = pll_ext(p);
  if (!x || !x->ctx)
  {
    pll_set_error(PLL_ERROR_GPU_UNAVAILABLE, "%s: no MI355X context behind this partition; this library has no CPU path", who);
    return fail_insertion();
  }

  /* inputs current on the device: the model, every named matrix, every named end once */
  unsigned int lo = subtree_matrix_index, hi = subtree_matrix_index;
  matrix_span(candidates, count, &lo, &hi);
  unsigned char *seen = (unsigned char *)calloc((size_t)p->nodes + p->scale_buffers + 1, 1);
  pllgpu_insertion_t *dev = (pllgpu_insertion_t *)malloc(sizeof(pllgpu_insertion_t) * count);
  if (!seen || !dev)
  {
    free(seen);
    free(dev);
    pll_set_error(PLL_ERROR_MEM_ALLOC, "%s: out of memory", who);
    return fail_insertion();
  }
  unsigned char *seen_scaler = seen + p->nodes;
  int ok = pll_flush_model(p, x) && pll_flush_pmatrix(p, x, lo, hi) &&
           prepare_once(p, x, seen, seen_scaler, subtree_clv_index, subtree_scaler_index) &&
           prepare_candidates(p, x, seen, seen_scaler, candidates, count, dev);
  free(seen);
  if (!ok)
  {
    free(dev);
    return fail_insertion();
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
    return fail_as(name);
  }
  if (!query_count || !count) return PLL_SUCCESS;
  if (!query_tip_indices || !candidates || !lnl || !freqs_indices)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: query_tip_indices, candidates, lnl or freqs_indices is NULL", name);
    return fail_as(name);
  }
  for (i = 0; i < query_count; ++i)
    if (query_tip_indices[i] >= p->tips)
    {
      pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: query %u: %u is no tip of the partition", name, i, query_tip_indices[i]);
      return fail_as(name);
    }
  if (pendant_matrix_index >= p->prob_matrices)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: the pendant matrix index is out of range", name);
    return fail_as(name);
  }
  if ((i = first_bad_candidate(p, candidates, count)) < count)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: candidate %u has an index out of range", name, i);
    return fail_as(name);
  }
  for (k = 0; k < p->rate_cats; ++k)
    if (freqs_indices[k] >= p->rate_matrices)
    {
      pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: freqs_indices[%u] out of range", name, k);
      return fail_as(name);
    }
  if (pll_repeats_enabled(p))
  {
    pll_set_error(PLL_ERROR_GPU_UNSUPPORTED, "%s: PLL_ATTRIB_SITE_REPEATS partitions are not supported", name);
    return fail_as(name);
  }
  if (p->attributes & PLL_ATTRIB_AB_MASK)
  {
    pll_set_error(PLL_ERROR_GPU_UNSUPPORTED, "%s: the ascertainment-bias correction needs pll_compute_edge_loglikelihood", name);
    return fail_as(name);
  }
  for (i = 0; i < query_count; ++i)
    if (!pll_tip_by_codes(p, query_tip_indices[i]))
    {
      /* the kernel reads a query as one byte per site */
      pll_set_error(PLL_ERROR_GPU_UNSUPPORTED, "%s: query %u: tip %u is not held as codes; set it again with pll_set_tip_states", name, i,
                    query_tip_indices[i]);
      return fail_as(name);
    }
  pll_amd_ext_t *x = pll_ext(p);
  if (!x || !x->ctx)
  {
    pll_set_error(PLL_ERROR_GPU_UNAVAILABLE, "%s: no MI355X context behind this partition; this library has no CPU path", name);
    return fail_as(name);
  }

  /* inputs current on the device: the model, every named matrix, every named end and every query tip once */
  unsigned int lo = pendant_matrix_index, hi = pendant_matrix_index;
  matrix_span(candidates, count, &lo, &hi);
  unsigned char *seen = (unsigned char *)calloc((size_t)p->nodes + p->scale_buffers + 1, 1);
  pllgpu_insertion_t *dev = (pllgpu_insertion_t *)malloc(sizeof(pllgpu_insertion_t) * count);
  if (!seen || !dev)
  {
    free(seen);
    free(dev);
    pll_set_error(PLL_ERROR_MEM_ALLOC, "%s: out of memory", name);
    return fail_as(name);
  }
  unsigned char *seen_scaler = seen + p->nodes;
  int ok = pll_flush_model(p, x) && pll_flush_pmatrix(p, x, lo, hi);
  for (i = 0; ok && i < query_count; ++i) ok = prepare_once(p, x, seen, seen_scaler, query_tip_indices[i], PLL_SCALE_BUFFER_NONE);
  ok = ok && prepare_candidates(p, x, seen, seen_scaler, candidates, count, dev);
  free(seen);
  if (!ok)
  {
    free(dev);
    return fail_as(name);
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
