/* ancestral.c - pll_compute_node_ancestral / pll_compute_node_ancestral_extbuf (src/likelihood.c:639-823) and the
 * stream-ordered pll_gpu_node_ancestral_async.
 *
 * The reference forms the product CLV (identity x node) * (P x other) in temp_clv with pll_core_update_partial_{ii,ti},
 * then mixes rates and frequencies and normalises per site. Here one kernel does all of it (kernels_ancestral.h); the
 * three scratch buffers of the _extbuf form are checked for NULL like the reference does and otherwise left alone.
 *
 * Which end is read how: the other end is read as tip codes whenever the device holds it as codes (a
 * PLL_ATTRIB_PATTERN_TIP tip, src/likelihood.c:688-704, or one of this library's compact indicator tips) - P is
 * applied on that side in the caller's orientation, so nothing is swapped. The node's end is always a CLV: a compact
 * tip there is given its dense CLV back; a PATTERN_TIP tip has none (the reference dereferences NULL) and is refused.
 *
 * Deliberate difference from the reference: with PLL_ATTRIB_RATE_SCALERS the per-rate scaling counts of both ends are
 * honoured (min + capped differences, like the root likelihood and the ascertainment terms, likelihood.c); the
 * reference ignores them and rescales each rate of the product on its own (src/likelihood.c:711-722, :730-743). */
#include "pll_internal.h"

static int node_ancestral(const char *who, pll_partition_t *p, unsigned int node_clv_index, int node_scaler_index,
                          unsigned int other_clv_index, int other_scaler_index, unsigned int matrix_index,
                          const unsigned int *freqs_indices, double *host_out, void *device_out)
{
  if (pll_repeats_enabled(p))
  {
    pll_set_error(PLL_ERROR_EINVAL, "Site repeats are not compatible with ancestral state reconstruction!");
    return PLL_FAILURE;
  }
  if (!freqs_indices)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: freqs_indices is NULL", who);
    return PLL_FAILURE;
  }
  if (node_clv_index >= p->nodes || other_clv_index >= p->nodes || matrix_index >= p->prob_matrices ||
      node_scaler_index >= (int)p->scale_buffers || other_scaler_index >= (int)p->scale_buffers)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: index out of range", who);
    return PLL_FAILURE;
  }
  if (pll_is_pattern_tip(p, node_clv_index))
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: the node is a pattern tip, it has no CLV", who);
    return PLL_FAILURE;
  }
  pll_amd_ext_t *x = pll_ext(p);
  if (!x || !x->ctx)
  {
    pll_set_error(PLL_ERROR_GPU_UNAVAILABLE, "%s: no MI355X context behind this partition; this library has no CPU path", who);
    return PLL_FAILURE;
  }
  pll_tip_densify(p, node_clv_index); /* a compact tip as the node: its dense CLV */
  const int otip = pll_tip_by_codes(p, other_clv_index);
  if (!pll_flush_model(p, x) || !pll_flush_pmatrix(p, x, matrix_index, matrix_index) ||
      !pll_prepare_end(p, x, node_clv_index, node_scaler_index) ||
      !pll_prepare_end(p, x, other_clv_index, other_scaler_index))
    return PLL_FAILURE;

  pllgpu_edge_t e;
  memset(&e, 0, sizeof e);
  e.parent_clv = node_clv_index;
  e.parent_scaler = node_scaler_index;
  e.child_clv = other_clv_index;
  e.child_scaler = otip ? PLL_SCALE_BUFFER_NONE : other_scaler_index;
  e.child_is_tip = otip;
  e.matrix = matrix_index;
  e.freqs_indices = freqs_indices;
  if (pllgpu_node_ancestral(x->ctx, &e, host_out, device_out) != 0)
  {
    pll_set_gpu_error(who);
    return PLL_FAILURE;
  }
  return PLL_SUCCESS;
}

int pll_compute_node_ancestral_extbuf(pll_partition_t *partition, unsigned int node_clv_index, int node_scaler_index,
                                      unsigned int other_clv_index, int other_scaler_index, unsigned int pmatrix_index,
                                      const unsigned int *freqs_indices, double *ancestral, double *temp_clv,
                                      unsigned int *temp_scaler, double *ident_pmat)
{
  if (!partition || !ancestral)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "Parameter value is NULL!");
    return PLL_FAILURE;
  }
  if (!temp_clv || !temp_scaler || !ident_pmat)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "NULL buffer pointer");
    return PLL_FAILURE;
  }
  return node_ancestral("pll_compute_node_ancestral_extbuf", partition, node_clv_index, node_scaler_index, other_clv_index,
                        other_scaler_index, pmatrix_index, freqs_indices, ancestral, NULL);
}

int pll_compute_node_ancestral(pll_partition_t *partition, unsigned int node_clv_index, int node_scaler_index,
                               unsigned int other_clv_index, int other_scaler_index, unsigned int matrix_index,
                               const unsigned int *freqs_indices, double *ancestral)
{
  if (!partition || !ancestral)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "Parameter value is NULL!");
    return PLL_FAILURE;
  }
  return node_ancestral("pll_compute_node_ancestral", partition, node_clv_index, node_scaler_index, other_clv_index,
                        other_scaler_index, matrix_index, freqs_indices, ancestral, NULL);
}

int pll_gpu_node_ancestral_async(pll_partition_t *partition, unsigned int node_clv_index, int node_scaler_index,
                                 unsigned int other_clv_index, int other_scaler_index, unsigned int matrix_index,
                                 const unsigned int *freqs_indices, void *device_ancestral)
{
  if (!partition || !device_ancestral)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "Parameter value is NULL!");
    return PLL_FAILURE;
  }
  return node_ancestral("pll_gpu_node_ancestral_async", partition, node_clv_index, node_scaler_index, other_clv_index,
                        other_scaler_index, matrix_index, freqs_indices, NULL, device_ancestral);
}
