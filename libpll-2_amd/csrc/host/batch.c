/* batch.c - what the batched calls share on the host side: pll_gpu_insertion_loglikelihoods and
 * pll_gpu_placement_loglikelihoods (insertion.c), the quartet calls (quartet.c) and pll_gpu_branch_derivatives
 * (derivatives.c); DESIGN.md section 5.6 says what such a call is made of.
 *
 * Each of them validates its whole list before anything is flushed or launched, refuses what the device layer has no
 * kernel for, brings every end its list names up to date on the device once, and follows one error convention: pll_errno
 * and pll_errmsg set, one line on stderr, PLL_FAILURE. The list checks stay with the calls; the rest is here. */
#include "pll_internal.h"

int pll_batch_fail(const char *who)
{
  fprintf(stderr, "libpll_amd: %s: [%d] %s\n", who, pll_errno, pll_errmsg);
  return PLL_FAILURE;
}

int pll_batch_end_in_range(const pll_partition_t *p, unsigned int clv, int scaler, unsigned int matrix)
{
  return clv < p->nodes && matrix < p->prob_matrices && scaler >= PLL_SCALE_BUFFER_NONE && scaler < (int)p->scale_buffers;
}

int pll_batch_refusals(const char *who, const pll_partition_t *p, const char *reference_call)
{
  if (pll_repeats_enabled(p))
  {
    /* the nodes a kernel forms in registers or LDS have no class map */
    pll_set_error(PLL_ERROR_GPU_UNSUPPORTED, "%s: PLL_ATTRIB_SITE_REPEATS partitions are not supported", who);
    return pll_batch_fail(who);
  }
  if (p->attributes & PLL_ATTRIB_AB_MASK)
  {
    if (reference_call)
      pll_set_error(PLL_ERROR_GPU_UNSUPPORTED, "%s: the ascertainment-bias correction needs %s", who, reference_call);
    else
      pll_set_error(PLL_ERROR_GPU_UNSUPPORTED, "%s: partitions with an ascertainment-bias correction are not supported", who);
    return pll_batch_fail(who);
  }
  return PLL_SUCCESS;
}

int pll_batch_device(const char *who, const pll_partition_t *p, pll_amd_ext_t **ext)
{
  pll_amd_ext_t *x = pll_ext(p);
  if (!x || !x->ctx)
  {
    pll_set_error(PLL_ERROR_GPU_UNAVAILABLE, "%s: no MI355X context behind this partition; this library has no CPU path", who);
    return pll_batch_fail(who);
  }
  *ext = x;
  return PLL_SUCCESS;
}

int pll_batch_refusals_and_device(const char *who, const pll_partition_t *p, const char *reference_call, pll_amd_ext_t **ext)
{
  return pll_batch_refusals(who, p, reference_call) && pll_batch_device(who, p, ext);
}

void *pll_batch_alloc(const char *who, const pll_partition_t *p, pll_batch_seen_t *seen, size_t list_bytes)
{
  void *list = malloc(list_bytes);
  seen->clv = (unsigned char *)calloc((size_t)p->nodes + p->scale_buffers + 1, 1);
  seen->scaler = seen->clv ? seen->clv + p->nodes : NULL;
  if (seen->clv && list) return list;
  pll_batch_seen_free(seen);
  free(list);
  pll_set_error(PLL_ERROR_MEM_ALLOC, "%s: out of memory", who);
  pll_batch_fail(who);
  return NULL;
}

void pll_batch_seen_free(pll_batch_seen_t *seen)
{
  free(seen->clv);
  seen->clv = seen->scaler = NULL;
}

int pll_batch_prepare_once(pll_partition_t *p, pll_amd_ext_t *x, pll_batch_seen_t *seen, unsigned int clv, int scaler)
{
  const int wants_scaler = scaler >= 0 && !pll_tip_by_codes(p, clv);
  if (seen->clv[clv] && !(wants_scaler && !seen->scaler[scaler])) return 1;
  seen->clv[clv] = 1;
  if (wants_scaler) seen->scaler[scaler] = 1;
  return pll_prepare_end(p, x, clv, scaler);
}
