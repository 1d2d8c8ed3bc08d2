/* parsimony.c - the bit-parallel Fitch parsimony entry points (src/fast_parsimony.c, src/parsimony.c:69-115).
 *
 * Host side of the feature: site classification and tip packing (pll_fastparsimony_init - one-off integer set-up, done
 * here in C and uploaded once), the side table that ties a pll_parsimony_t to its device record, dependency levels of an
 * operation list, argument checks, the host mirror and pll_parsimony_destroy. The arithmetic of every update and score
 * runs on the device (csrc/hip/kernels_parsimony.h behind the pllgpu_pars_* calls).
 *
 * pll_parsimony_t has no spare field and must stay byte-identical to the reference's, and - unlike a partition - a
 * structure that reaches pll_parsimony_destroy may have been allocated by another library; so nothing is hidden behind
 * the struct: the device record lives in a table keyed by the structure's address. */
#include <limits.h>
#include <pthread.h>

#include "pll_internal.h"

#define PLL_BITVECTOR_SIZE 32u
/* src/pll.h:77-78 */
#define PLL_STAT(x) ((pll_hardware.init || pll_hardware_probe()) && pll_hardware.x)

typedef struct pars_record
{
  const pll_parsimony_t *key;
  pllgpu_pars_t *dev; /* NULL: made under PLL_AMD_HOST_ONLY=1 */
  unsigned int nodes; /* tips + 3 * inner_nodes */
  /* scratch of pll_fastparsimony_update_vectors, [nodes] each: the latest level that writes / reads a node */
  int *wlevel, *rlevel;
  pllgpu_pars_op_t *ops, *sorted;
  unsigned int ops_cap;
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
  if (!r)
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
    r->ops = (pllgpu_pars_op_t *)malloc(count * sizeof *r->ops);
    r->sorted = (pllgpu_pars_op_t *)malloc(count * sizeof *r->sorted);
    r->ops_cap = r->ops && r->sorted ? count : 0;
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
    for (i = 0; i < count; ++i) r->sorted[start[r->ops[i].level]++] = r->ops[i];
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

int pll_gpu_sync_parsimony(pll_parsimony_t *pars, int node)
{
  static const char *who = "pll_gpu_sync_parsimony";
  pars_record_t *r = need_device(pars, who);
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
  return r && r->dev ? pllgpu_pars_last_launch_count(r->dev) : 0;
}

int pll_gpu_synchronize_parsimony(pll_parsimony_t *pars)
{
  static const char *who = "pll_gpu_synchronize_parsimony";
  pars_record_t *r = need_device(pars, who);
  if (!r) return PLL_FAILURE;
  if (pllgpu_pars_synchronize(r->dev) != 0)
  {
    pll_set_gpu_error(who);
    return PLL_FAILURE;
  }
  return PLL_SUCCESS;
}
