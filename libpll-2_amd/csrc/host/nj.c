/* nj.c - pll_gpu_nj_tree / pll_gpu_distance_tree (include/pll_amd.h; csrc/hip/kernels_nj.h):
 * neighbour-joining and BIONJ trees joined on the device, from a matrix of the caller's or from the tips of a partition;
 * pll_gpu_nj_trees / pll_gpu_bootstrap_distance_trees (section 5.17): many of them in one call, from many matrices or
 * from replicate weights drawn on the device.
 *
 * Host side: the argument checks, the one pass over the upper triangle that refuses entries that are negative or not
 * finite, and the error convention of batch.c. The join itself has no host part: pllamd/nj.py restates it in numpy. */
#include <math.h>

#include "pll_internal.h"

static int tree_arguments(const char *who, unsigned int count, unsigned int flags)
{
  if (count < 3)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: %u nodes; a tree joins at least 3", who, count);
    return pll_batch_fail(who);
  }
  if (flags & ~PLL_GPU_NJ_BIONJ)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: unknown flag bits %#x", who, flags & ~PLL_GPU_NJ_BIONJ);
    return pll_batch_fail(who);
  }
  return PLL_SUCCESS;
}

static int device_failed(const char *who, int rc)
{
  if (rc == PLLGPU_ENODEVICE)
    pll_set_error(PLL_ERROR_GPU_UNAVAILABLE, "%s: %s; this library has no CPU path", who, pllgpu_last_error());
  else if (rc == PLLGPU_ENOMEM)
    pll_set_error(PLL_ERROR_MEM_ALLOC, "%s: %s", who, pllgpu_last_error());
  else
  {
    pll_set_gpu_error(who); /* (prints its own line) */
    return PLL_FAILURE;
  }
  return pll_batch_fail(who);
}

/* the one pass over the upper triangles of `replicates` matrices; `batched`: the message names the matrix */
static int matrix_entries(const char *who, const double *distances, unsigned int count, unsigned int replicates, int batched)
{
  unsigned int b, x, y;
  for (b = 0; b < replicates; ++b)
    for (x = 0; x < count; ++x)
      for (y = x + 1; y < count; ++y)
      {
        const double d = distances[((size_t)b * count + x) * count + y];
        if (!(d >= 0) || !isfinite(d))
        {
          if (batched)
            pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: distances[%u][%u][%u] = %g is negative or not finite", who, b, x, y, d);
          else
            pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: distances[%u][%u] = %g is negative or not finite", who, x, y, d);
          return pll_batch_fail(who);
        }
      }
  return PLL_SUCCESS;
}

int pll_gpu_nj_tree(const double *distances, unsigned int count, unsigned int flags, int device, int *parent, double *length)
{
  static const char who[] = "pll_gpu_nj_tree";
  if (!distances || !parent || !length)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: distances, parent or length is NULL", who);
    return pll_batch_fail(who);
  }
  if (!tree_arguments(who, count, flags) || !matrix_entries(who, distances, count, 1, 0)) return PLL_FAILURE;
  const int rc = pllgpu_nj_tree(device, distances, count, flags, parent, length);
  return rc ? device_failed(who, rc) : PLL_SUCCESS;
}

int pll_gpu_nj_trees(const double *distances, unsigned int count, unsigned int replicates, unsigned int flags, int device, int *parent,
                     double *length)
{
  static const char who[] = "pll_gpu_nj_trees";
  if (!distances || !parent || !length)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: distances, parent or length is NULL", who);
    return pll_batch_fail(who);
  }
  if (!tree_arguments(who, count, flags)) return PLL_FAILURE;
  if (!replicates) return PLL_SUCCESS;
  if (!matrix_entries(who, distances, count, replicates, 1)) return PLL_FAILURE;
  const int rc = pllgpu_nj_trees(device, distances, count, replicates, flags, parent, length);
  return rc ? device_failed(who, rc) : PLL_SUCCESS;
}

int pll_gpu_distance_tree(pll_partition_t *p, const unsigned int *tips, unsigned int count, const unsigned int *params_indices,
                          const pll_gpu_newton_t *options, unsigned int flags, int *parent, double *length, double *distances_out)
{
  static const char who[] = "pll_gpu_distance_tree";
  if (!p || !parent || !length)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: partition, parent or length is NULL", who);
    return pll_batch_fail(who);
  }
  pll_amd_ext_t *x = NULL;
  pllgpu_newton_t opt;
  /* (no tip makes no list: its checks have nothing to look at, and count < 3 refuses it) */
  if (count && !pll_distances_check(who, p, tips, count, params_indices, options, &x)) return PLL_FAILURE;
  if (!tree_arguments(who, count, flags)) return PLL_FAILURE;
  if (!pll_distances_flush(who, p, x, tips, count, params_indices, options, &opt)) return PLL_FAILURE;
  const int rc = pllgpu_distance_tree(x->ctx, tips, count, params_indices, &opt, flags, parent, length, distances_out);
  return rc ? device_failed(who, rc) : PLL_SUCCESS;
}

int pll_gpu_bootstrap_distance_trees(pll_partition_t *p, const unsigned int *tips, unsigned int count, const unsigned int *params_indices,
                                     const pll_gpu_newton_t *options, unsigned int flags, unsigned long long seed, unsigned int first_replicate,
                                     unsigned int replicates, const pll_gpu_bootstrap_trees_t *out)
{
  static const char who[] = "pll_gpu_bootstrap_distance_trees";
  unsigned int i;
  if (!p || !out || !out->parent || !out->length)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: partition, out, out->parent or out->length is NULL", who);
    return pll_batch_fail(who);
  }
  if (!replicates) return PLL_SUCCESS;
  pll_amd_ext_t *x = NULL;
  pllgpu_newton_t opt;
  if (count && !pll_distances_check(who, p, tips, count, params_indices, options, &x)) return PLL_FAILURE;
  if (!tree_arguments(who, count, flags)) return PLL_FAILURE;
  /* a replicate of no draws is none: the refusal of pll_gpu_draw_replicate_weights, made here before anything is flushed */
  unsigned long long wsum = 0;
  for (i = 0; i < p->sites; ++i) wsum += p->pattern_weights[i];
  if (!wsum)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: the pattern weights add up to 0; a replicate needs a sum in [1, 2^32)", who);
    return pll_batch_fail(who);
  }
  if (!pll_distances_flush(who, p, x, tips, count, params_indices, options, &opt)) return PLL_FAILURE;
  const pllgpu_bootstrap_trees_t dev = {out->parent, out->length, out->distances, out->status, out->weights};
  const int rc = pllgpu_bootstrap_distance_trees(x->ctx, tips, count, params_indices, &opt, flags, seed, first_replicate, replicates, &dev);
  return rc ? device_failed(who, rc) : PLL_SUCCESS;
}

int pll_gpu_bootstrap_last_times(const pll_partition_t *p, double *ms)
{
  pll_amd_ext_t *x = p ? pll_ext(p) : NULL;
  if (!x || !x->ctx || !ms) return PLL_FAILURE;
  return pllgpu_bootstrap_last_times(x->ctx, ms) == 0 ? PLL_SUCCESS : PLL_FAILURE;
}

unsigned int pll_gpu_nj_last_launch_count(void) { return pllgpu_nj_last_launch_count(); }

double pll_gpu_nj_last_device_ms(void) { return pllgpu_nj_last_device_ms(); }
