/* parsimony.c - the parsimony entry points: bit-parallel Fitch (src/fast_parsimony.c, src/parsimony.c:69-115) and, in the
 * second half of the file, weighted (Sankoff) parsimony (src/parsimony.c:24-67, :117-383; kernels_sankoff.h behind the
 * pllgpu_spars_* calls). Both kinds share the side table, the dependency levels and pll_parsimony_destroy.
 *
 * Fitch:
 * Host side of the feature: site classification and tip packing (pll_fastparsimony_init - one-off integer set-up, done
 * here in C and uploaded once), the side table that ties a pll_parsimony_t to its device record, dependency levels of an
 * operation list, argument checks, the host mirror and pll_parsimony_destroy. The arithmetic of every update and score
 * runs on the device (csrc/hip/kernels_parsimony.h behind the pllgpu_pars_* calls).
 *
 * pll_parsimony_t has no spare field and must stay byte-identical to the reference's, and - unlike a partition - a
 * structure that reaches pll_parsimony_destroy may have been allocated by another library; so nothing is hidden behind
 * the struct: the device record lives in a table keyed by the structure's address. */
#include <limits.h>
#include <math.h>
#include <pthread.h>

#include "pll_internal.h"

#define PLL_BITVECTOR_SIZE 32u
/* src/pll.h:77-78 */
#define PLL_STAT(x) ((pll_hardware.init || pll_hardware_probe()) && pll_hardware.x)

enum { KIND_FAST, KIND_WEIGHTED };

typedef struct pars_record
{
  const pll_parsimony_t *key;
  int kind;            /* KIND_FAST: pll_fastparsimony_init made it; KIND_WEIGHTED: pll_parsimony_create */
  pllgpu_pars_t *dev;  /* fast; NULL: made under PLL_AMD_HOST_ONLY=1 */
  pllgpu_spars_t *sdev; /* weighted; NULL: made under PLL_AMD_HOST_ONLY=1 */
  unsigned int nodes; /* fast: tips + 3 * inner_nodes; weighted: what the level scratch holds (score or ancestral buffers) */
  /* scratch of assign_levels, [nodes] each: the latest level that writes / reads a node */
  int *wlevel, *rlevel;
  pllgpu_pars_op_t *ops, *sorted;
  unsigned int *order; /* sorted[i] is entry order[i] of the list */
  unsigned int ops_cap;
  /* weighted only */
  unsigned int score_nodes;      /* tips + score_buffers */
  unsigned char *host_newer;     /* [score_nodes] sbuffer[i] was written on the host after its last upload */
  unsigned int *indices;         /* [score_nodes] scratch: the buffers of an upload or a download */
  int eager;                     /* PLL_AMD_EAGER_MIRROR=1 */
  struct pars_record *next;
} pars_record_t;

static pars_record_t *g_records;
static pthread_mutex_t g_records_lock = PTHREAD_MUTEX_INITIALIZER;

static pars_record_t *record_find(const pll_parsimony_t *pars, int unlink)
{
  pars_record_t **at, *r = NULL;
  pthread_mutex_lock(&g_records_lock);
  for (at = &g_records; *at; at = &(*at)->next)
    if ((*at)->key == pars)
    {
      r = *at;
      if (unlink) *at = r->next;
      break;
    }
  pthread_mutex_unlock(&g_records_lock);
  return r;
}

static void record_add(pars_record_t *r)
{
  pthread_mutex_lock(&g_records_lock);
  r->next = g_records;
  g_records = r;
  pthread_mutex_unlock(&g_records_lock);
}

static void record_free(pars_record_t *r)
{
  if (!r) return;
  if (r->dev) pllgpu_pars_destroy(r->dev);
  if (r->sdev) pllgpu_spars_destroy(r->sdev);
  free(r->host_newer);
  free(r->indices);
  free(r->order);
  free(r->wlevel);
  free(r->rlevel);
  free(r->ops);
  free(r->sorted);
  free(r);
}

/* the record of a structure that a device call may use, or NULL with pll_errno set */
static pars_record_t *need_device(const pll_parsimony_t *pars, const char *who)
{
  pars_record_t *r = pars ? record_find(pars, 0) : NULL;
  if (!r || r->kind != KIND_FAST)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: structure was not created by this library's pll_fastparsimony_init", who);
    return NULL;
  }
  if (!r->dev)
  {
    pll_set_error(PLL_ERROR_GPU_UNAVAILABLE, "%s: no MI355X behind this structure (PLL_AMD_HOST_ONLY); this library has no CPU path", who);
    return NULL;
  }
  return r;
}

static int index_ok(const pars_record_t *r, unsigned int index, const char *who)
{
  if (index < r->nodes) return 1;
  pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: score index %u out of range (%u vectors)", who, index, r->nodes);
  return 0;
}

/* ---- site classification (src/fast_parsimony.c:82-194, :369-403) ------------------------------------------------- */

static int cmp_u32(const void *a, const void *b)
{
  const unsigned int x = *(const unsigned int *)a, y = *(const unsigned int *)b;
  return (x > y) - (x < y);
}

/* The reference counts, per site, how many distinct tip characters occur more than once (informative: at least two)
 * and how many occur exactly once (*singleton: the mutations a non-informative site costs). A "character" is the tip's
 * code under PLL_ATTRIB_PATTERN_TIP and otherwise the bit string of its CLV entry, so an ambiguity code is a character
 * of its own. The reference tallies in a table of 256 or 2^states counters; sorting the tips' keys gives the same two
 * numbers without the table. keys: scratch of `tips` words. */
static int check_informative(const pll_partition_t *p, unsigned int site, unsigned int *keys, unsigned int *singleton)
{
  unsigned int i, j, count = 0;
  *singleton = 0;
  for (i = 0; i < p->tips; ++i)
  {
    if (p->attributes & PLL_ATTRIB_PATTERN_TIP) keys[i] = p->tipchars[i][site];
    else
    {
      const double *clv = p->clv[i] + (size_t)site * p->states_padded * p->rate_cats;
      unsigned int c = 0;
      for (j = 0; j < p->states; ++j) c = (c << 1) | (unsigned int)(clv[j]);
      keys[i] = c;
    }
  }
  qsort(keys, p->tips, sizeof *keys, cmp_u32);
  for (i = 0; i < p->tips; i = j)
  {
    for (j = i + 1; j < p->tips && keys[j] == keys[i]; ++j) {}
    if (j - i > 1) ++count;
    else ++*singleton;
  }
  return count > 1;
}

/* ---- tip packing (src/fast_parsimony.c:196-367) -------------------------------------------------------------------- */

static void fill_tip_vector(const pll_partition_t *p, const pll_parsimony_t *pars, unsigned int tip, unsigned int *val)
{
  const unsigned int states = pars->states, words = pars->packedvector_count;
  unsigned int *vec = pars->packedvector[tip];
  unsigned int j, k, m, bitcount = 0, w = 0;
  memset(val, 0, states * sizeof *val);
  for (j = 0; j < pars->sites; ++j)
  {
    if (!pars->informative[j]) continue;
    pll_state_t mask = 0;
    if (pars->attributes & PLL_ATTRIB_PATTERN_TIP)
    {
      mask = p->tipchars[tip][j];
      if (states != 4) mask = p->tipmap[mask];
    }
    else
    {
      const double *clv = p->clv[tip] + (size_t)j * p->states_padded * p->rate_cats;
      for (k = 0; k < states; ++k)
        if ((int)(clv[k])) mask |= (pll_state_t)1 << k;
    }
    for (m = 0; m < p->pattern_weights[j]; ++m)
    {
      pll_state_t c = mask;
      for (k = 0; k < states; ++k, c >>= 1)
        if (c & 1) val[k] |= 1u << bitcount;
      if (++bitcount == PLL_BITVECTOR_SIZE)
      {
        for (k = 0; k < states; ++k)
        {
          vec[(size_t)k * words + w] = val[k];
          val[k] = 0;
        }
        ++w;
        bitcount = 0;
      }
    }
  }
  /* the rest of the last word, and the words the rounding added: ones (they match everything and cost nothing) */
  if (bitcount)
  {
    for (k = 0; k < states; ++k) vec[(size_t)k * words + w] = val[k] | (~0u << bitcount);
    ++w;
  }
  for (; w < words; ++w)
    for (k = 0; k < states; ++k) vec[(size_t)k * words + w] = ~0u;
}

static void free_host_fields(pll_parsimony_t *pars)
{
  /* src/parsimony.c:69-115, every branch of it: also what frees a structure another library made */
  unsigned int i;
  const unsigned int nodes = pars->tips + 3 * pars->inner_nodes;
  if (pars->packedvector)
  {
    for (i = 0; i < nodes; ++i) pll_aligned_free(pars->packedvector[i]);
    free(pars->packedvector);
  }
  free(pars->node_cost);
  free(pars->informative);
  if (pars->sbuffer)
  {
    for (i = 0; i < pars->score_buffers + pars->tips; ++i) free(pars->sbuffer[i]);
    free(pars->sbuffer);
  }
  if (pars->anc_states)
  {
    for (i = pars->tips; i < pars->ancestral_buffers + pars->tips; ++i) free(pars->anc_states[i]);
    free(pars->anc_states);
  }
  free(pars->score_matrix);
  free(pars);
}

pll_parsimony_t *pll_fastparsimony_init(const pll_partition_t *p)
{
  unsigned int i, bitcount = 0, words, singletons = 0, noninformative = 0;
  if (!p)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "pll_fastparsimony_init: partition is NULL");
    return NULL;
  }
  if (p->states > 20 && !(p->attributes & PLL_ATTRIB_PATTERN_TIP))
  {
    pll_set_error(PLL_ERROR_STEPWISE_UNSUPPORTED, "Use PLL_ATTRIB_PATTERN_TIP for more than 20 states.");
    return NULL;
  }
  if (pll_repeats_enabled(p))
  {
    pll_set_error(PLL_ERROR_GPU_UNSUPPORTED, "pll_fastparsimony_init: not available for a PLL_ATTRIB_SITE_REPEATS partition; "
                                             "build the parsimony structure from a partition without site repeats");
    return NULL;
  }
  pll_amd_ext_t *x = pll_ext(p);
  if (!x)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "pll_fastparsimony_init: partition was not created by libpll_amd");
    return NULL;
  }
  if (!(p->attributes & PLL_ATTRIB_PATTERN_TIP) && x->ctx)
    for (i = 0; i < p->tips; ++i) /* a tip CLV that is newer on the device (none, unless the caller computed into it) */
      if (!pll_gpu_sync_clv((pll_partition_t *)p, i)) return NULL;

  pll_parsimony_t *pars = (pll_parsimony_t *)calloc(1, sizeof *pars);
  pars_record_t *r = (pars_record_t *)calloc(1, sizeof *r);
  unsigned int *scratch = (unsigned int *)malloc(((size_t)p->tips + p->states + 1) * sizeof *scratch);
  if (!pars || !r || !scratch) goto nomem;
  pars->tips = p->tips;
  pars->inner_nodes = p->tips - 1;
  pars->sites = p->sites;
  pars->attributes = p->attributes;
  pars->states = p->states;
  pars->alignment = p->alignment;
  r->key = pars;
  r->nodes = pars->tips + 3 * pars->inner_nodes;

  /* informative sites; the rest cost their singletons, once and for all (src/fast_parsimony.c:369-403) */
  pars->informative = (int *)malloc((p->sites ? p->sites : 1) * sizeof(int));
  if (!pars->informative) goto nomem;
  for (i = 0; i < p->sites; ++i)
  {
    pars->informative[i] = check_informative(p, i, scratch, &singletons);
    if (pars->informative[i]) bitcount += p->pattern_weights[i];
    else
    {
      ++noninformative;
      pars->const_cost += singletons * p->pattern_weights[i];
    }
  }
  pars->informative_count = p->sites - noninformative;

  /* words per state, rounded as the reference's vector kernels need it (src/fast_parsimony.c:247-264) */
  words = bitcount / PLL_BITVECTOR_SIZE + (bitcount % PLL_BITVECTOR_SIZE != 0);
  if ((pars->attributes & PLL_ATTRIB_ARCH_SSE) && PLL_STAT(sse3_present)) words = (words + 3) & 0xFFFFFFFCu;
  if ((pars->attributes & PLL_ATTRIB_ARCH_AVX) && PLL_STAT(avx_present)) words = (words + 7) & 0xFFFFFFF8u;
  if ((pars->attributes & PLL_ATTRIB_ARCH_AVX2) && PLL_STAT(avx2_present)) words = (words + 7) & 0xFFFFFFF8u;
  pars->packedvector_count = words;

  pars->node_cost = (unsigned int *)calloc(r->nodes, sizeof(unsigned int));
  pars->packedvector = (unsigned int **)calloc(r->nodes, sizeof(unsigned int *));
  r->wlevel = (int *)malloc(r->nodes * sizeof(int));
  r->rlevel = (int *)malloc(r->nodes * sizeof(int));
  if (!pars->node_cost || !pars->packedvector || !r->wlevel || !r->rlevel) goto nomem;
  for (i = 0; i < r->nodes; ++i)
  {
    const size_t bytes = (size_t)pars->states * words * sizeof(unsigned int);
    pars->packedvector[i] = (unsigned int *)pll_aligned_alloc(bytes, pars->alignment);
    if (!pars->packedvector[i]) goto nomem;
    if (i < pars->tips) fill_tip_vector(p, pars, i, scratch + p->tips);
    else memset(pars->packedvector[i], 0, bytes);
  }
  free(scratch);
  scratch = NULL;

  if (x->ctx)
  {
    r->dev = pllgpu_pars_create(pllgpu_context_device(x->ctx), pars->states, words, r->nodes);
    if (!r->dev || pllgpu_pars_upload(r->dev, 0, pars->tips, pars->packedvector) != 0)
    {
      pll_set_gpu_error("pll_fastparsimony_init");
      record_free(r);
      free_host_fields(pars);
      return NULL;
    }
  }
  record_add(r);
  return pars;

nomem:
  pll_set_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate parsimony structures.");
  free(scratch);
  record_free(r);
  if (pars) free_host_fields(pars);
  return NULL;
}

void pll_parsimony_destroy(pll_parsimony_t *pars)
{
  if (!pars) return;
  record_free(record_find(pars, 1));
  free_host_fields(pars);
}

/* ---- updates ------------------------------------------------------------------------------------------------------- */

/* Levels such that running level after level, everything of a level at once, equals running the list in order: an entry
 * goes behind the writers of its children (read after write), behind every earlier reader of its parent (write after
 * read) and behind its parent's earlier writer (write after write). Its own reads do not count against its own write:
 * a lane loads what it needs of the children before it stores (kernels_parsimony.h). Returns the ops sorted by level. */
static const pllgpu_pars_op_t *assign_levels(pars_record_t *r, const pll_pars_buildop_t *ops, unsigned int count)
{
  unsigned int i, nlevels = 0;
  if (count > r->ops_cap)
  {
    free(r->ops);
    free(r->sorted);
    free(r->order);
    r->ops = (pllgpu_pars_op_t *)malloc(count * sizeof *r->ops);
    r->sorted = (pllgpu_pars_op_t *)malloc(count * sizeof *r->sorted);
    r->order = (unsigned int *)malloc(count * sizeof *r->order);
    r->ops_cap = r->ops && r->sorted && r->order ? count : 0;
    if (!r->ops_cap) return NULL;
  }
  for (i = 0; i < r->nodes; ++i) r->wlevel[i] = r->rlevel[i] = -1;
  for (i = 0; i < count; ++i)
  {
    const unsigned int pa = ops[i].parent_score_index, c1 = ops[i].child1_score_index, c2 = ops[i].child2_score_index;
    int level = r->wlevel[c1] + 1;
    if (r->wlevel[c2] + 1 > level) level = r->wlevel[c2] + 1;
    if (r->rlevel[pa] + 1 > level) level = r->rlevel[pa] + 1;
    if (r->wlevel[pa] + 1 > level) level = r->wlevel[pa] + 1;
    if (r->rlevel[c1] < level) r->rlevel[c1] = level;
    if (r->rlevel[c2] < level) r->rlevel[c2] = level;
    /* (a self-referencing entry has just marked its parent as read at its own level: the next writer goes behind it) */
    r->wlevel[pa] = level;
    r->ops[i].parent = pa;
    r->ops[i].child1 = c1;
    r->ops[i].child2 = c2;
    r->ops[i].level = (unsigned int)level;
    if ((unsigned int)level + 1 > nlevels) nlevels = (unsigned int)level + 1;
  }
  /* stable counting sort by level: entries of a level keep the list's order */
  {
    unsigned int *start = (unsigned int *)calloc((size_t)nlevels + 1, sizeof *start);
    if (!start) return NULL;
    for (i = 0; i < count; ++i) ++start[r->ops[i].level + 1];
    for (i = 0; i < nlevels; ++i) start[i + 1] += start[i];
    for (i = 0; i < count; ++i)
    {
      const unsigned int at = start[r->ops[i].level]++;
      r->sorted[at] = r->ops[i];
      r->order[at] = i;
    }
    free(start);
  }
  return r->sorted;
}

void pll_fastparsimony_update_vectors(pll_parsimony_t *pars, const pll_pars_buildop_t *ops, unsigned int count)
{
  static const char *who = "pll_fastparsimony_update_vectors";
  unsigned int i;
  pars_record_t *r = need_device(pars, who);
  if (!r)
  {
    fprintf(stderr, "libpll_amd: %s\n", pll_errmsg); /* a void entry point of the reference API: be loud as well */
    return;
  }
  if (!count) return;
  if (!ops)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: operations is NULL", who);
    return;
  }
  for (i = 0; i < count; ++i)
    if (!index_ok(r, ops[i].parent_score_index, who) || !index_ok(r, ops[i].child1_score_index, who) ||
        !index_ok(r, ops[i].child2_score_index, who))
      return;
  const pllgpu_pars_op_t *sorted = assign_levels(r, ops, count);
  if (!sorted)
  {
    pll_set_error(PLL_ERROR_MEM_ALLOC, "%s: cannot allocate the level schedule", who);
    return;
  }
  if (pllgpu_pars_update(r->dev, sorted, count) != 0) pll_set_gpu_error(who);
}

void pll_fastparsimony_update_vector(pll_parsimony_t *pars, const pll_pars_buildop_t *op)
{
  pll_fastparsimony_update_vectors(pars, op, 1);
}

void pll_fastparsimony_update_vector_4x4(pll_parsimony_t *pars, const pll_pars_buildop_t *op)
{
  pll_fastparsimony_update_vectors(pars, op, 1);
}

/* ---- scores -------------------------------------------------------------------------------------------------------- */

int pll_gpu_fastparsimony_edge_scores(const pll_parsimony_t *pars, const unsigned int *pairs, unsigned int count, unsigned int *scores)
{
  static const char *who = "pll_gpu_fastparsimony_edge_scores";
  unsigned int i;
  pars_record_t *r = need_device(pars, who);
  if (!r) return PLL_FAILURE;
  if (!count) return PLL_SUCCESS;
  if (!pairs || !scores)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: Parameter value is NULL!", who);
    return PLL_FAILURE;
  }
  for (i = 0; i < 2 * count; ++i)
    if (!index_ok(r, pairs[i], who)) return PLL_FAILURE;
  if (pllgpu_pars_edge_scores(r->dev, pairs, count, pars->const_cost, scores) != 0)
  {
    pll_set_gpu_error(who);
    return PLL_FAILURE;
  }
  return PLL_SUCCESS;
}

int pll_gpu_fastparsimony_insertion_scores(const pll_parsimony_t *pars, unsigned int node, const unsigned int *edges, unsigned int count,
                                           unsigned int *scores)
{
  static const char *who = "pll_gpu_fastparsimony_insertion_scores";
  unsigned int i;
  pars_record_t *r = need_device(pars, who);
  if (!r) return PLL_FAILURE;
  if (!index_ok(r, node, who)) return PLL_FAILURE;
  if (!count) return PLL_SUCCESS;
  if (!edges || !scores)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: Parameter value is NULL!", who);
    return PLL_FAILURE;
  }
  for (i = 0; i < 2 * count; ++i)
    if (!index_ok(r, edges[i], who)) return PLL_FAILURE;
  if (pllgpu_pars_insertion_scores(r->dev, node, edges, count, pars->const_cost, scores) != 0)
  {
    pll_set_gpu_error(who);
    return PLL_FAILURE;
  }
  return PLL_SUCCESS;
}

unsigned int pll_fastparsimony_edge_score(const pll_parsimony_t *pars, unsigned int node1_score_index, unsigned int node2_score_index)
{
  const unsigned int pair[2] = {node1_score_index, node2_score_index};
  unsigned int score = UINT_MAX;
  if (!pll_gpu_fastparsimony_edge_scores(pars, pair, 1, &score)) return UINT_MAX;
  return score;
}

unsigned int pll_fastparsimony_edge_score_4x4(const pll_parsimony_t *pars, unsigned int node1_score_index, unsigned int node2_score_index)
{
  return pll_fastparsimony_edge_score(pars, node1_score_index, node2_score_index);
}

unsigned int pll_fastparsimony_root_score(const pll_parsimony_t *pars, unsigned int root_index)
{
  static const char *who = "pll_fastparsimony_root_score";
  unsigned int cost = 0;
  pars_record_t *r = need_device(pars, who);
  if (!r || !index_ok(r, root_index, who)) return UINT_MAX;
  if (pllgpu_pars_node_cost(r->dev, root_index, &cost) != 0)
  {
    pll_set_gpu_error(who);
    return UINT_MAX;
  }
  return cost + pars->const_cost;
}

/* ---- mirror, bookkeeping ------------------------------------------------------------------------------------------- */

static int weighted_sync(pars_record_t *r, pll_parsimony_t *pars, int node, const char *who);

int pll_gpu_sync_parsimony(pll_parsimony_t *pars, int node)
{
  static const char *who = "pll_gpu_sync_parsimony";
  pars_record_t *r = pars ? record_find(pars, 0) : NULL;
  if (r && r->kind == KIND_WEIGHTED) return weighted_sync(r, pars, node, who);
  r = need_device(pars, who);
  if (!r) return PLL_FAILURE;
  if (node >= 0 && !index_ok(r, (unsigned int)node, who)) return PLL_FAILURE;
  if (pllgpu_pars_download(r->dev, node < 0 ? 0u : (unsigned int)node, node < 0 ? r->nodes : 1u, pars->packedvector, pars->node_cost) != 0)
  {
    pll_set_gpu_error(who);
    return PLL_FAILURE;
  }
  return PLL_SUCCESS;
}

unsigned int pll_gpu_fastparsimony_last_launch_count(const pll_parsimony_t *pars)
{
  pars_record_t *r = pars ? record_find(pars, 0) : NULL;
  if (r && r->sdev) return pllgpu_spars_last_launch_count(r->sdev);
  return r && r->dev ? pllgpu_pars_last_launch_count(r->dev) : 0;
}

static int weighted_device(const pars_record_t *r, const char *who);

int pll_gpu_synchronize_parsimony(pll_parsimony_t *pars)
{
  static const char *who = "pll_gpu_synchronize_parsimony";
  pars_record_t *r = pars ? record_find(pars, 0) : NULL;
  if (r && r->kind == KIND_WEIGHTED)
  {
    if (!weighted_device(r, who)) return PLL_FAILURE;
    if (pllgpu_spars_synchronize(r->sdev) != 0)
    {
      pll_set_gpu_error(who);
      return PLL_FAILURE;
    }
    return PLL_SUCCESS;
  }
  r = need_device(pars, who);
  if (!r) return PLL_FAILURE;
  if (pllgpu_pars_synchronize(r->dev) != 0)
  {
    pll_set_gpu_error(who);
    return PLL_FAILURE;
  }
  return PLL_SUCCESS;
}

/* ==== weighted (Sankoff) parsimony (src/parsimony.c:24-67, :117-383) =================================================
 * Host side: the fields the reference leaves, argument checks (the whole list before anything is uploaded or launched),
 * dependency levels, the stale-mirror bookkeeping and the two character tables of a reconstruction. Every add and min
 * runs on the device. Order of the checks in every call: the structure (PLL_ERROR_PARAM_INVALID), the arguments
 * (PLL_ERROR_PARAM_INVALID), the device (PLL_ERROR_GPU_UNAVAILABLE for a host-only structure). */

static pars_record_t *weighted_record(const pll_parsimony_t *pars, const char *who)
{
  pars_record_t *r = pars ? record_find(pars, 0) : NULL;
  if (!r || r->kind != KIND_WEIGHTED)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: structure was not created by this library's pll_parsimony_create", who);
    return NULL;
  }
  pllgpu_spars_clear_launch_count(r->sdev); /* a call that fails its checks has launched nothing */
  return r;
}

static int weighted_device(const pars_record_t *r, const char *who)
{
  if (r->sdev) return 1;
  pll_set_error(PLL_ERROR_GPU_UNAVAILABLE, "%s: no MI355X behind this structure (PLL_AMD_HOST_ONLY); this library has no CPU path", who);
  return 0;
}

static int score_index_ok(const pars_record_t *r, unsigned int index, const char *who)
{
  if (index < r->score_nodes) return 1;
  pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: score index %u out of range (%u buffers)", who, index, r->score_nodes);
  return 0;
}

static int anc_index_ok(const pll_parsimony_t *pars, unsigned int index, const char *who)
{
  if (index >= pars->tips && index - pars->tips < pars->ancestral_buffers) return 1;
  pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: ancestral index %u out of range [%u, %u)", who, index, pars->tips,
                pars->tips + pars->ancestral_buffers);
  return 0;
}

pll_parsimony_t *pll_parsimony_create(unsigned int tips, unsigned int states, unsigned int sites, const double *score_matrix,
                                      unsigned int score_buffers, unsigned int ancestral_buffers)
{
  static const char *who = "pll_parsimony_create";
  unsigned int i;
  if (states < 1 || states > 64)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: %u states (1..64: pll_state_t has 64 bits)", who, states);
    return NULL;
  }
  if (!tips || !sites || !score_matrix || tips + score_buffers < tips || tips + ancestral_buffers < tips)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: tips = %u, sites = %u, score_matrix %s", who, tips, sites, score_matrix ? "given" : "NULL");
    return NULL;
  }
  pll_parsimony_t *pars = (pll_parsimony_t *)calloc(1, sizeof *pars);
  pars_record_t *r = (pars_record_t *)calloc(1, sizeof *r);
  if (!pars || !r) goto nomem;
  /* src/parsimony.c:135-199: the passed parameters, a private matrix, zeroed buffers; every fast-parsimony field zero */
  pars->tips = tips;
  pars->states = states;
  pars->sites = sites;
  pars->score_buffers = score_buffers;
  pars->ancestral_buffers = ancestral_buffers;
  r->key = pars;
  r->kind = KIND_WEIGHTED;
  r->score_nodes = tips + score_buffers;
  r->nodes = r->score_nodes > ancestral_buffers ? r->score_nodes : ancestral_buffers;
  r->eager = pll_env_flag("PLL_AMD_EAGER_MIRROR");
  pars->score_matrix = (double *)calloc((size_t)states * states, sizeof(double));
  pars->sbuffer = (double **)calloc(r->score_nodes, sizeof(double *));
  pars->anc_states = (unsigned int **)calloc((size_t)tips + ancestral_buffers, sizeof(unsigned int *));
  r->wlevel = (int *)malloc(r->nodes * sizeof(int));
  r->rlevel = (int *)malloc(r->nodes * sizeof(int));
  r->host_newer = (unsigned char *)calloc(r->score_nodes, 1);
  r->indices = (unsigned int *)malloc(r->score_nodes * sizeof(unsigned int));
  if (!pars->score_matrix || !pars->sbuffer || !pars->anc_states || !r->wlevel || !r->rlevel || !r->host_newer || !r->indices) goto nomem;
  memcpy(pars->score_matrix, score_matrix, (size_t)states * states * sizeof(double));
  for (i = 0; i < r->score_nodes; ++i)
    if (!(pars->sbuffer[i] = (double *)calloc((size_t)sites * states, sizeof(double)))) goto nomem;
  for (i = tips; i < tips + ancestral_buffers; ++i)
    if (!(pars->anc_states[i] = (unsigned int *)calloc(sites, sizeof(unsigned int)))) goto nomem;

  /* There is no CPU arithmetic behind this library: without a device the structure is refused, as pll_partition_create
   * refuses a partition, unless the caller asks for a host-only shell */
  if (!pll_env_flag("PLL_AMD_HOST_ONLY"))
  {
    r->sdev = pllgpu_spars_create(-1, states, sites, r->score_nodes, ancestral_buffers, pars->score_matrix);
    if (!r->sdev)
    {
      pll_set_error(PLL_ERROR_GPU_UNAVAILABLE, "MI355X context: %s", pllgpu_last_error());
      record_free(r);
      free_host_fields(pars);
      return NULL;
    }
  }
  record_add(r);
  return pars;

nomem:
  pll_set_error(PLL_ERROR_MEM_ALLOC, "Unable to allocate enough memory.");
  record_free(r);
  if (pars) free_host_fields(pars);
  return NULL;
}

int pll_set_parsimony_sequence(pll_parsimony_t *pars, unsigned int tip_index, const pll_state_t *map, const char *sequence)
{
  static const char *who = "pll_set_parsimony_sequence";
  unsigned int i, j;
  pars_record_t *r = weighted_record(pars, who);
  if (!r) return PLL_FAILURE;
  if (!map || !sequence)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: Parameter value is NULL!", who);
    return PLL_FAILURE;
  }
  if (!score_index_ok(r, tip_index, who)) return PLL_FAILURE;
  const unsigned int states = pars->states;
  double *tipstate = pars->sbuffer[tip_index];
  /* src/parsimony.c:37-42: infinity is the highest score in the matrix plus one */
  double inf = pars->score_matrix[0];
  for (i = 1; i < states * states; ++i)
    if (pars->score_matrix[i] > inf) inf = pars->score_matrix[i];
  inf++;
  r->host_newer[tip_index] = 1; /* also when the sequence turns out illegal half way: the host copy has changed */
  for (i = 0; i < pars->sites; ++i)
  {
    pll_state_t c = map[(unsigned char)sequence[i]];
    if (c == 0)
    {
      pll_set_error(PLL_ERROR_TIPDATA_ILLEGALSTATE, "Illegal state code in tip \"%c\"", sequence[i]);
      printf("%s\n", pll_errmsg); /* src/parsimony.c:50 */
      return PLL_FAILURE;
    }
    for (j = 0; j < states; ++j, c >>= 1) tipstate[j] = (c & 1) ? 0 : inf;
    tipstate += states;
  }
  return PLL_SUCCESS;
}

int pll_gpu_parsimony_invalidate(pll_parsimony_t *pars, unsigned int index)
{
  static const char *who = "pll_gpu_parsimony_invalidate";
  pars_record_t *r = weighted_record(pars, who);
  if (!r || !score_index_ok(r, index, who)) return PLL_FAILURE;
  r->host_newer[index] = 1;
  return PLL_SUCCESS;
}

/* every buffer the host wrote since its last upload goes up, all of them in one staging copy */
static int flush_stale(pars_record_t *r, const pll_parsimony_t *pars, const char *who)
{
  unsigned int i, n = 0;
  for (i = 0; i < r->score_nodes; ++i)
    if (r->host_newer[i]) r->indices[n++] = i;
  if (!n) return 1;
  if (pllgpu_spars_upload(r->sdev, r->indices, n, pars->sbuffer) != 0)
  {
    pll_set_gpu_error(who);
    return 0;
  }
  memset(r->host_newer, 0, r->score_nodes);
  return 1;
}

double pll_parsimony_build(pll_parsimony_t *pars, const pll_pars_buildop_t *ops, unsigned int count)
{
  static const char *who = "pll_parsimony_build";
  unsigned int i, n = 0;
  double score = -INFINITY;
  pars_record_t *r = weighted_record(pars, who);
  if (!r) return -INFINITY;
  if (!ops || !count)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: empty operation list", who);
    return -INFINITY;
  }
  for (i = 0; i < count; ++i)
    if (!score_index_ok(r, ops[i].parent_score_index, who) || !score_index_ok(r, ops[i].child1_score_index, who) ||
        !score_index_ok(r, ops[i].child2_score_index, who))
      return -INFINITY;
  if (!weighted_device(r, who)) return -INFINITY;
  const pllgpu_pars_op_t *sorted = assign_levels(r, ops, count);
  if (!sorted)
  {
    pll_set_error(PLL_ERROR_MEM_ALLOC, "%s: cannot allocate the level schedule", who);
    return -INFINITY;
  }
  if (!flush_stale(r, pars, who)) return -INFINITY;
  if (pllgpu_spars_build(r->sdev, sorted, count, ops[count - 1].parent_score_index, &score) != 0)
  {
    pll_set_gpu_error(who);
    return -INFINITY;
  }
  if (r->eager)
  {
    /* assign_levels has left the level of the last write in wlevel[]: the parents of the list */
    for (i = 0; i < r->score_nodes; ++i)
      if (r->wlevel[i] >= 0) r->indices[n++] = i;
    if (pllgpu_spars_download(r->sdev, r->indices, n, pars->sbuffer) != 0)
    {
      pll_set_gpu_error(who);
      return -INFINITY;
    }
  }
  return score;
}

double pll_parsimony_score(pll_parsimony_t *pars, unsigned int score_buffer_index)
{
  static const char *who = "pll_parsimony_score";
  double score = -INFINITY;
  pars_record_t *r = weighted_record(pars, who);
  if (!r || !score_index_ok(r, score_buffer_index, who) || !weighted_device(r, who)) return -INFINITY;
  if (!flush_stale(r, pars, who)) return -INFINITY;
  if (pllgpu_spars_score(r->sdev, score_buffer_index, &score) != 0)
  {
    pll_set_gpu_error(who);
    return -INFINITY;
  }
  return score;
}

static unsigned int state_ctz(pll_state_t x)
{
  return (unsigned int)__builtin_ctzll(x);
}

void pll_parsimony_reconstruct(pll_parsimony_t *pars, const pll_state_t *map, const pll_pars_recop_t *ops, unsigned int count)
{
  static const char *who = "pll_parsimony_reconstruct";
  unsigned int i, lo, hi, tables[512];
  pll_pars_buildop_t *deps = NULL;
  pllgpu_spars_recop_t *recops = NULL;
  unsigned int **wanted = NULL;
  pars_record_t *r = weighted_record(pars, who);
  if (!r) goto loud;
  if (!map || !ops)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: Parameter value is NULL!", who);
    goto loud;
  }
  if (!count) return;
  for (i = 0; i < count; ++i)
  {
    if (!score_index_ok(r, ops[i].node_score_index, who) || !anc_index_ok(pars, ops[i].node_ancestral_index, who)) goto loud;
    /* the first operation has no parent: the reference never reads those two fields (src/parsimony.c:336-349) */
    if (i && (!score_index_ok(r, ops[i].parent_score_index, who) || !anc_index_ok(pars, ops[i].parent_ancestral_index, who))) goto loud;
  }
  if (!weighted_device(r, who)) goto loud;

  /* src/parsimony.c:327-334, in its loop order: of two characters with the same single bit the later one wins. The
   * second table is what the reference computes per site, PLL_STATE_CTZ(map[character]); a character without a state in
   * range (a hole in the reverse map leads to one) counts as state 0 instead of indexing out of bounds */
  memset(tables, 0, sizeof tables);
  for (i = 0; i < 256; ++i)
    if (__builtin_popcountll(map[i]) == 1) tables[state_ctz(map[i])] = i;
  for (i = 0; i < 256; ++i)
    tables[256 + i] = map[i] && state_ctz(map[i]) < pars->states ? state_ctz(map[i]) : 0;

  /* levels over the ancestral buffers: an operation reads its parent's and writes its own */
  deps = (pll_pars_buildop_t *)malloc(count * sizeof *deps);
  recops = (pllgpu_spars_recop_t *)malloc(count * sizeof *recops);
  wanted = (unsigned int **)calloc(pars->ancestral_buffers, sizeof *wanted);
  if (!deps || !recops || !wanted) goto nomem;
  for (i = 0; i < count; ++i)
  {
    deps[i].parent_score_index = ops[i].node_ancestral_index - pars->tips;
    deps[i].child1_score_index = deps[i].child2_score_index = (i ? ops[i].parent_ancestral_index : ops[i].node_ancestral_index) - pars->tips;
  }
  const pllgpu_pars_op_t *sorted = assign_levels(r, deps, count);
  if (!sorted) goto nomem;
  lo = hi = sorted[0].parent;
  for (i = 0; i < count; ++i)
  {
    const pll_pars_recop_t *op = &ops[r->order[i]];
    recops[i].node_score = op->node_score_index;
    recops[i].node_ancestral = sorted[i].parent;
    recops[i].parent_score = r->order[i] ? op->parent_score_index : op->node_score_index;
    recops[i].parent_ancestral = sorted[i].child1;
    recops[i].root = r->order[i] == 0;
    recops[i].level = sorted[i].level;
    if (sorted[i].parent < lo) lo = sorted[i].parent;
    if (sorted[i].parent > hi) hi = sorted[i].parent;
    wanted[sorted[i].parent] = pars->anc_states[pars->tips + sorted[i].parent];
  }
  if (!flush_stale(r, pars, who)) goto done;
  /* anc_states[] of every node the list names comes back before the call returns: it is the call's result */
  if (pllgpu_spars_reconstruct(r->sdev, recops, count, tables) != 0 ||
      pllgpu_spars_download_ancestral(r->sdev, lo, hi - lo + 1, wanted) != 0)
  {
    pll_set_gpu_error(who);
    goto done;
  }
  goto done;

nomem:
  pll_set_error(PLL_ERROR_MEM_ALLOC, "%s: cannot allocate the level schedule", who);
loud:
  fprintf(stderr, "libpll_amd: %s\n", pll_errmsg); /* a void entry point of the reference API: be loud as well */
done:
  free(deps);
  free(recops);
  free(wanted);
}

int pll_gpu_parsimony_insertion_scores(const pll_parsimony_t *pars, unsigned int node, const unsigned int *edges, unsigned int count,
                                       double *scores)
{
  static const char *who = "pll_gpu_parsimony_insertion_scores";
  unsigned int i;
  pars_record_t *r = weighted_record(pars, who);
  if (!r || !score_index_ok(r, node, who)) return PLL_FAILURE;
  if (count && (!edges || !scores))
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: Parameter value is NULL!", who);
    return PLL_FAILURE;
  }
  for (i = 0; i < 2 * count; ++i)
    if (!score_index_ok(r, edges[i], who)) return PLL_FAILURE;
  if (!weighted_device(r, who)) return PLL_FAILURE;
  if (!count) return PLL_SUCCESS;
  if (!flush_stale(r, pars, who)) return PLL_FAILURE;
  if (pllgpu_spars_insertion_scores(r->sdev, node, edges, count, scores) != 0)
  {
    pll_set_gpu_error(who);
    return PLL_FAILURE;
  }
  return PLL_SUCCESS;
}

/* pll_gpu_sync_parsimony of a weighted structure: score buffer `node` and, where it has one, ancestral buffer `node`
 * (node < 0: all of both). A score buffer whose host copy is the newer one is left alone. */
static int weighted_sync(pars_record_t *r, pll_parsimony_t *pars, int node, const char *who)
{
  unsigned int i, n = 0;
  const unsigned int u = (unsigned int)node;
  const int has_anc = node >= 0 && u >= pars->tips && u - pars->tips < pars->ancestral_buffers;
  if (node >= 0 && u >= r->score_nodes && !has_anc)
  {
    pll_set_error(PLL_ERROR_PARAM_INVALID, "%s: index %u names neither a score buffer nor an ancestral buffer", who, u);
    return PLL_FAILURE;
  }
  if (!weighted_device(r, who)) return PLL_FAILURE;
  for (i = 0; i < r->score_nodes; ++i)
    if ((node < 0 || i == u) && !r->host_newer[i]) r->indices[n++] = i;
  if (pllgpu_spars_download(r->sdev, r->indices, n, pars->sbuffer) != 0 ||
      (node < 0 && pllgpu_spars_download_ancestral(r->sdev, 0, pars->ancestral_buffers, pars->anc_states + pars->tips) != 0) ||
      (has_anc && pllgpu_spars_download_ancestral(r->sdev, u - pars->tips, 1, pars->anc_states + pars->tips) != 0))
  {
    pll_set_gpu_error(who);
    return PLL_FAILURE;
  }
  return PLL_SUCCESS;
}
