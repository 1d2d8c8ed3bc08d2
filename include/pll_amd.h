/*
 * pll_amd.h - public C interface of the MI355X (gfx950) build of the libpll-2 partial-likelihood
 * hot path.
 *
 * This header is written from the ABI record in SURVEY.md section 8b, not transcribed from the
 * reference header. It declares ONLY what the hot path needs, with struct layouts that are
 * byte-identical to the reference (x86-64 LP64) so that a caller compiled against the
 * reference's own pll.h can link against libpll_amd.so unchanged. Every declaration cites the
 * reference declaration it replaces (paths relative to the reference checkout).
 *
 * The library computes on the GPU only. There is no CPU kernel behind these entry points: if no
 * gfx950 device (or the HIP code object) is available, pll_partition_create() fails with
 * pll_errno = PLL_ERROR_GPU_UNAVAILABLE instead of silently falling back.
 */
#ifndef PLL_AMD_H_
#define PLL_AMD_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status / limits (src/pll.h:82-110) --------------------------------------------------- */
#define PLL_FAILURE 0
#define PLL_SUCCESS 1
#define PLL_FALSE 0
#define PLL_TRUE 1

#define PLL_ALIGNMENT_CPU 8
#define PLL_ALIGNMENT_SSE 16
#define PLL_ALIGNMENT_AVX 32
#define PLL_ASCII_SIZE 256

/* 2^256 and its inverse, exact in binary64 (src/pll.h:96-97) */
#define PLL_SCALE_FACTOR 0x1p256
#define PLL_SCALE_THRESHOLD 0x1p-256
#define PLL_SCALE_BUFFER_NONE (-1)
#define PLL_SCALE_RATE_MAXDIFF 4 /* src/pll.h:104 */

/* ---- attribute word (src/pll.h:112-137) --------------------------------------------------- */
/* The ARCH bits only select the *host-visible layout* (states_padded, alignment) so existing
 * callers that pass ARCH_AVX2 keep seeing the padding they expect; arithmetic always runs on
 * the MI355X. */
#define PLL_ATTRIB_ARCH_CPU 0u
#define PLL_ATTRIB_ARCH_SSE (1u << 0)
#define PLL_ATTRIB_ARCH_AVX (1u << 1)
#define PLL_ATTRIB_ARCH_AVX2 (1u << 2)
#define PLL_ATTRIB_ARCH_AVX512 (1u << 3)
#define PLL_ATTRIB_ARCH_MASK 0xFu
#define PLL_ATTRIB_PATTERN_TIP (1u << 4)
#define PLL_ATTRIB_AB_LEWIS (1u << 5)
#define PLL_ATTRIB_AB_FELSENSTEIN (2u << 5)
#define PLL_ATTRIB_AB_STAMATAKIS (3u << 5)
#define PLL_ATTRIB_AB_MASK (7u << 5)
#define PLL_ATTRIB_AB_FLAG (1u << 8)
#define PLL_ATTRIB_RATE_SCALERS (1u << 9)
#define PLL_ATTRIB_SITE_REPEATS (1u << 10)
#define PLL_REPEATS_LOOKUP_SIZE 2000000u
#define PLL_ATTRIB_MASK ((1u << 11) - 1)

/* ---- error codes (subset of src/pll.h:154-190 that this path can raise) -------------------- */
#define PLL_ERROR_MEM_ALLOC 112
#define PLL_ERROR_PARAM_INVALID 113
#define PLL_ERROR_TIPDATA_ILLEGALSTATE 114
#define PLL_ERROR_TIPDATA_ILLEGALFUNCTION 115
#define PLL_ERROR_INVAR_INCOMPAT 117
#define PLL_ERROR_INVAR_PROPORTION 118
#define PLL_ERROR_INVAR_PARAMINDEX 119
#define PLL_ERROR_INVAR_NONEFOUND 120
#define PLL_ERROR_AB_INVALIDMETHOD 121
#define PLL_ERROR_AB_NOSUPPORT 122
#define PLL_ERROR_STEPWISE_UNSUPPORTED 129 /* src/pll.h:186 */
#define PLL_ERROR_EINVAL 130
#define PLL_ERROR_MSA_EMPTY 131
#define PLL_ERROR_MSA_MAP_INVALID 132
/* new, outside the reference's range: device problems are reported through the same
 * pll_errno / pll_errmsg convention */
#define PLL_ERROR_GPU_UNAVAILABLE 900
#define PLL_ERROR_GPU_RUNTIME 901
#define PLL_ERROR_GPU_UNSUPPORTED 902

#define PLL_GAMMA_RATES_MEAN 0
#define PLL_GAMMA_RATES_MEDIAN 1

/* ---- types ------------------------------------------------------------------------------- */
typedef unsigned long long pll_state_t; /* src/pll.h:217: one bit per state, <= 64 states */

struct pll_repeats;

/* src/pll.h:241-288; sizeof == 232, offsets asserted in csrc/host/abi_check.c */
typedef struct pll_partition
{
  unsigned int tips;
  unsigned int clv_buffers;
  unsigned int nodes;
  unsigned int states;
  unsigned int sites;
  unsigned int pattern_weight_sum;
  unsigned int rate_matrices;
  unsigned int prob_matrices;
  unsigned int rate_cats;
  unsigned int scale_buffers;
  unsigned int attributes;
  size_t alignment;
  unsigned int states_padded;
  double **clv;                  /* host mirror of the device CLVs, see pll_gpu_sync_* below */
  double **pmatrix;
  double *rates;
  double *rate_weights;
  double **subst_params;
  unsigned int **scale_buffer;   /* host mirror of the device scalers */
  double **frequencies;
  double *prop_invar;
  int *invariant;
  unsigned int *pattern_weights;
  int *eigen_decomp_valid;
  double **eigenvecs;
  double **inv_eigenvecs;
  double **eigenvals;
  unsigned int maxstates;
  unsigned char **tipchars;
  unsigned char *charmap;
  double *ttlookup;              /* kept NULL: the device kernels need no tip-tip table */
  pll_state_t *tipmap;
  int asc_bias_alloc;
  int asc_additional_sites;
  struct pll_repeats *repeats;
} pll_partition_t;

/* src/pll.h:290-321; sizeof == 104 */
typedef struct pll_repeats
{
  unsigned int **pernode_site_id;
  unsigned int **pernode_id_site;
  unsigned int *pernode_ids;
  unsigned int *perscale_ids;
  unsigned int *pernode_allocated_clvs;
  unsigned int (*enable_repeats)(struct pll_partition *partition, unsigned int left_clv,
                                 unsigned int right_clv);
  void (*reallocate_repeats)(struct pll_partition *partition, unsigned int parent,
                             int scaler_index, unsigned int sites_to_alloc);
  unsigned int *lookup_buffer;
  unsigned int *toclean_buffer;
  unsigned int *id_site_buffer;
  double *bclv_buffer;
  unsigned int lookup_buffer_size;
  char *charmap;
} pll_repeats_t;

/* src/pll.h:325-335; eight 4-byte fields, sizeof == 32 */
typedef struct pll_operation
{
  unsigned int parent_clv_index;
  int parent_scaler_index;
  unsigned int child1_clv_index;
  unsigned int child1_matrix_index;
  int child1_scaler_index;
  unsigned int child2_clv_index;
  unsigned int child2_matrix_index;
  int child2_scaler_index;
} pll_operation_t;

/* src/pll.h:347-354 */
typedef struct pll_msa_s
{
  int count;
  int length;
  char **sequence;
  char **label;
} pll_msa_t;

/* src/pll.h:468-492; sizeof == 104, offsets asserted in csrc/host/abi_check.c. pll_fastparsimony_init fills the "fast
 * unweighted parsimony" fields and leaves the weighted (Sankoff) ones zero; pll_parsimony_create does the opposite. */
typedef struct pll_parsimony_s
{
  unsigned int tips;
  unsigned int inner_nodes;
  unsigned int sites;
  unsigned int states;
  unsigned int attributes;
  size_t alignment;
  unsigned int **packedvector; /* host mirror of the device vectors, see pll_gpu_sync_parsimony below */
  unsigned int *node_cost;     /* host mirror of the device costs */
  unsigned int packedvector_count;
  unsigned int const_cost;
  int *informative;
  unsigned int informative_count;
  unsigned int score_buffers;
  unsigned int ancestral_buffers;
  double *score_matrix;
  double **sbuffer;            /* host mirror of the device score buffers, see "weighted parsimony" below */
  unsigned int **anc_states;   /* the result of pll_parsimony_reconstruct */
} pll_parsimony_t;

/* src/pll.h:495-500; three unsigned int, sizeof == 12 */
typedef struct pll_pars_buildop_s
{
  unsigned int parent_score_index;
  unsigned int child1_score_index;
  unsigned int child2_score_index;
} pll_pars_buildop_t;

/* src/pll.h:502-508; four unsigned int, sizeof == 16 */
typedef struct pll_pars_recop_s
{
  unsigned int node_score_index;
  unsigned int node_ancestral_index;
  unsigned int parent_score_index;
  unsigned int parent_ancestral_index;
} pll_pars_recop_t;

/* ---- printers used by the reference's examples and tests (src/pll.h:2590-2600, src/output.c) -- */
void pll_show_pmatrix(const pll_partition_t *partition, unsigned int index, unsigned int float_precision);
void pll_show_clv(const pll_partition_t *partition, unsigned int clv_index, int scaler_index, unsigned int float_precision);

/* ---- host feature record (src/pll.h:220-237, :555, :2694-2698; src/hardware.c) -------------- */
/* Callers test it (PLL_STAT(avx2_present), src/pll.h:77-78) before they ask for a PLL_ATTRIB_ARCH_* layout.
 * Here the bits describe the host CPU as the reference's probe does; they only ever select a host
 * LAYOUT (states_padded), the arithmetic runs on the device whatever they say. */
typedef struct pll_hardware_s
{
  int init;
  int altivec_present, mmx_present, sse_present, sse2_present, sse3_present, ssse3_present, sse41_present,
      sse42_present, popcnt_present, avx_present, avx2_present;
} pll_hardware_t;
extern __thread pll_hardware_t pll_hardware;
int pll_hardware_probe(void);   /* fills pll_hardware; returns PLL_SUCCESS */
void pll_hardware_dump(void);   /* prints the record */
void pll_hardware_ignore(void); /* marks every feature present */

/* ---- thread-local error state (src/pll.h:553-555, src/pll.c:24-25) ------------------------- */
extern __thread int pll_errno;
extern __thread char pll_errmsg[200];

/* ---- character maps callers hand to pll_set_tip_states (src/pll.h:557-560, src/maps.c) ----- */
extern const pll_state_t pll_map_bin[256];
extern const pll_state_t pll_map_nt[256];
extern const pll_state_t pll_map_gt10[256]; /* diploid genotypes, 10 unordered / 16 ordered states */
extern const pll_state_t pll_map_gt16[256];
extern const pll_state_t pll_map_aa[256];

/* ---- lifecycle (src/pll.h:638-648, src/pll.c:424-873) -------------------------------------- */
pll_partition_t *pll_partition_create(unsigned int tips, unsigned int clv_buffers,
                                      unsigned int states, unsigned int sites,
                                      unsigned int rate_matrices, unsigned int prob_matrices,
                                      unsigned int rate_cats, unsigned int scale_buffers,
                                      unsigned int attributes);
void pll_partition_destroy(pll_partition_t *partition);
void *pll_aligned_alloc(size_t size, size_t alignment); /* src/pll.h:778 */
void pll_aligned_free(void *ptr);                       /* src/pll.h:780 */

/* ---- site-pattern compression (src/pll.h:2499-2510, src/compress.c:171-410) ----------------- */
/* Merges identical alignment columns: the sequences are rewritten in place with the unique columns
 * (sorted lexicographically by encoded character, NUL-terminated), *length becomes their number,
 * the returned vector (malloc'ed, caller frees) holds their multiplicities; the _msa variant also
 * fills site_pattern_map[original site] = pattern index. The ordering and counting run on the
 * MI355X (csrc/hip/compress.hip); outputs are identical to the reference's. */
unsigned int *pll_compress_site_patterns(char **sequence, const pll_state_t *map, int count, int *length);
unsigned int *pll_compress_site_patterns_msa(pll_msa_t *msa, const pll_state_t *map,
                                             unsigned int *site_pattern_map);

/* ---- inputs (src/pll.h:650-661,746-758; src/pll.c:1026-1143; src/models.c:445-493) --------- */
int pll_set_tip_states(pll_partition_t *partition, unsigned int tip_index,
                       const pll_state_t *map, const char *sequence);
int pll_set_tip_clv(pll_partition_t *partition, unsigned int tip_index, const double *clv,
                    int padding);
void pll_set_pattern_weights(pll_partition_t *partition, const unsigned int *pattern_weights);
/* ascertainment-bias correction (src/pll.h:663-667, src/pll.c:1145-1200): the partition must have
 * been created with PLL_ATTRIB_AB_FLAG or an AB type; type = 0 | PLL_ATTRIB_AB_{LEWIS,FELSENSTEIN,
 * STAMATAKIS}. The correction enters pll_compute_{edge,root}_loglikelihood and
 * pll_compute_likelihood_derivatives (src/likelihood.c:24-120,191-268,342-440;
 * src/core_derivatives.c:851-924). Not combinable with PLL_ATTRIB_SITE_REPEATS (refused at creation). */
int pll_set_asc_bias_type(pll_partition_t *partition, int asc_bias_type);
void pll_set_asc_state_weights(pll_partition_t *partition, const unsigned int *state_weights);
void pll_set_frequencies(pll_partition_t *partition, unsigned int params_index,
                         const double *frequencies);
void pll_set_subst_params(pll_partition_t *partition, unsigned int params_index,
                          const double *params);
void pll_set_category_rates(pll_partition_t *partition, const double *rates);
void pll_set_category_weights(pll_partition_t *partition, const double *rate_weights);
int pll_update_invariant_sites_proportion(pll_partition_t *partition, unsigned int params_index,
                                          double prop_invar); /* src/models.c:495-540 */
int pll_update_invariant_sites(pll_partition_t *partition);  /* src/models.c:651-752 */
/* src/models.c:546-649: pattern-weighted number of invariant sites; state_inv_count[states] (or
 * NULL) receives the number of invariant patterns per state */
unsigned int pll_count_invariant_sites(pll_partition_t *partition, unsigned int *state_inv_count);

/* model side ("next" rows f2 of SURVEY section 8; host code, feeds the path) */
int pll_update_eigen(pll_partition_t *partition, unsigned int params_index); /* models.c:293 */
int pll_update_prob_matrices(pll_partition_t *partition, const unsigned int *params_indices,
                             const unsigned int *matrix_indices, const double *branch_lengths,
                             unsigned int count); /* src/models.c:412-443 */
int pll_compute_gamma_cats(double alpha, unsigned int categories, double *output_rates,
                           int rates_mode); /* src/gamma.c:220-292 */

/* ---- THE HOT PATH (src/pll.h:790-797,823-830) ---------------------------------------------- */
/* src/partials.c:237-291. Asynchronous: kernels are enqueued on the partition's HIP stream and
 * the call returns; results stay resident in HBM. */
void pll_update_partials(pll_partition_t *partition, const pll_operation_t *operations,
                         unsigned int count);
void pll_update_partials_rep(pll_partition_t *partition, const pll_operation_t *operations,
                             unsigned int count, unsigned int update_repeats);
/* src/likelihood.c:586-636. Synchronises the stream; returns -INFINITY (and sets pll_errno) on
 * a device error. persite_lnl may be NULL. */
double pll_compute_edge_loglikelihood(pll_partition_t *partition, unsigned int parent_clv_index,
                                      int parent_scaler_index, unsigned int child_clv_index,
                                      int child_scaler_index, unsigned int matrix_index,
                                      const unsigned int *freqs_indices, double *persite_lnl);
/* src/likelihood.c:122-189 ("next" row f3) */
double pll_compute_root_loglikelihood(pll_partition_t *partition, unsigned int clv_index,
                                      int scaler_index, const unsigned int *freqs_indices,
                                      double *persite_lnl);
/* src/pll.h:799-806, src/likelihood.c:758-823. Marginal ancestral state probabilities of the node whose CLV is
 * node_clv_index, oriented towards the node at other_clv_index across matrix_index: ancestral[n * states + j],
 * unpadded, each site's row sums to 1. One kernel and one device-to-host copy; synchronises. The other end may be
 * a tip of any kind; the node's end must have a CLV (a PLL_ATTRIB_PATTERN_TIP tip is refused with
 * PLL_ERROR_PARAM_INVALID where the reference dereferences NULL). Site repeats: PLL_ERROR_EINVAL, as in the
 * reference. prop_invar is ignored, as in the reference. Deliberate difference: with PLL_ATTRIB_RATE_SCALERS the
 * per-rate scaling counts of both ends are honoured (the reference ignores them, src/likelihood.c:711-743). */
int pll_compute_node_ancestral(pll_partition_t *partition, unsigned int node_clv_index, int node_scaler_index,
                               unsigned int other_clv_index, int other_scaler_index, unsigned int matrix_index,
                               const unsigned int *freqs_indices, double *ancestral);
/* src/pll.h:808-818, src/likelihood.c:639-756. The same; the three scratch buffers the reference computes in must
 * not be NULL (PLL_ERROR_PARAM_INVALID) but are neither read nor written here - the product CLV never leaves the
 * device's registers. Their contents after the call are unspecified. */
int pll_compute_node_ancestral_extbuf(pll_partition_t *partition, unsigned int node_clv_index, int node_scaler_index,
                                      unsigned int other_clv_index, int other_scaler_index, unsigned int pmatrix_index,
                                      const unsigned int *freqs_indices, double *ancestral, double *temp_clv,
                                      unsigned int *temp_scaler, double *ident_pmat);

/* ---- fast (bit-parallel Fitch) parsimony (src/pll.h:2559, :2574-2588; src/fast_parsimony.c, src/parsimony.c:69-115) --
 * What the reference's randomised stepwise addition is built from (src/stepwise.c:377-434, :507-512). Vectors and node
 * costs live in HBM; every result is an integer and equals the reference's exactly.
 *
 * pll_fastparsimony_init (src/pll.h:2574, src/fast_parsimony.c:523-555): classifies the sites (informative[],
 * informative_count, const_cost - ambiguity codes count as distinct characters, src/fast_parsimony.c:128-194), packs the
 * tips into states x packedvector_count words per node (pattern weights as repeated bits, the last word and the padding
 * words filled with ones; packedvector_count rounded to 4 or 8 words by the partition's PLL_ATTRIB_ARCH_* bits and
 * pll_hardware, src/fast_parsimony.c:247-264). This is one-off integer set-up, O(tips x sites): it runs ON THE HOST, in C,
 * and the tip vectors are uploaded once, in one copy. Tip data: partition->tipchars for a PLL_ATTRIB_PATTERN_TIP
 * partition; otherwise the host CLV mirror of each tip (the indicator CLVs pll_set_tip_states keeps there next to its
 * tip codes, or what pll_set_tip_clv stored; refreshed from the device first if the device copy is newer). More than 20
 * states without PLL_ATTRIB_PATTERN_TIP: NULL, PLL_ERROR_STEPWISE_UNSUPPORTED, as in the reference.
 * Deliberate differences: (1) a PLL_ATTRIB_SITE_REPEATS partition is refused with PLL_ERROR_GPU_UNSUPPORTED (the
 * applications build a separate partition without repeats for parsimony); (2) the inner-node mirrors packedvector[i]
 * are zero-filled at init, the reference leaves them uninitialised.
 * The structure is independent of the partition afterwards (the partition may be destroyed): it owns a device record -
 * the partition's device, a stream of its own, one block for all tips + 3 * inner_nodes vectors and the node costs - kept
 * in a side table keyed by the structure's address. Under PLL_AMD_HOST_ONLY=1 the host fields (tip vectors included) are
 * filled and no device is touched.
 *
 * Failure convention (the reference has none): a device failure sets pll_errno = PLL_ERROR_GPU_RUNTIME, an index >=
 * tips + 3 * inner_nodes or a structure this library did not create PLL_ERROR_PARAM_INVALID, a structure without a device
 * behind it (host-only) PLL_ERROR_GPU_UNAVAILABLE; a score is then UINT_MAX, an update does nothing. */
pll_parsimony_t *pll_fastparsimony_init(const pll_partition_t *partition);
/* src/pll.h:2576, src/fast_parsimony.c:709-717. Asynchronous on the structure's stream. The result equals executing the
 * list in order: the host assigns dependency levels that honour read-after-write, write-after-read and write-after-write
 * between the entries (an entry whose parent is one of its own children is legal, as in the reference), and every level
 * is ONE kernel launch - all its operations form one grid - plus one memset per call. */
void pll_fastparsimony_update_vectors(pll_parsimony_t *parsimony, const pll_pars_buildop_t *operations, unsigned int count);
/* src/pll.h:2587-2588, :2594-2595; src/fast_parsimony.c:458-521, :557-609: one-operation forms of the above. The reference's
 * _sse / _avx / _avx2 names are not exported, like those of the core functions. */
void pll_fastparsimony_update_vector(pll_parsimony_t *parsimony, const pll_pars_buildop_t *op);
void pll_fastparsimony_update_vector_4x4(pll_parsimony_t *parsimony, const pll_pars_buildop_t *op);
/* src/pll.h:2583, src/fast_parsimony.c:719-773: mismatches between the two vectors + both node costs + const_cost.
 * Synchronous: one launch and a 4-byte copy back. */
unsigned int pll_fastparsimony_edge_score(const pll_parsimony_t *parsimony, unsigned int node1_score_index,
                                          unsigned int node2_score_index);
unsigned int pll_fastparsimony_edge_score_4x4(const pll_parsimony_t *parsimony, unsigned int node1_score_index,
                                              unsigned int node2_score_index); /* src/pll.h:2590, src/fast_parsimony.c:405-456 */
/* src/pll.h:2580, src/fast_parsimony.c:776-781: node_cost[root_index] + const_cost. No launch, a 4-byte copy back. */
unsigned int pll_fastparsimony_root_score(const pll_parsimony_t *parsimony, unsigned int root_index);
/* src/pll.h:2559, src/parsimony.c:69-115. Releases the device record. A structure the library has no record of (one made
 * by another library's pll_parsimony_create or pll_fastparsimony_init, which reach this symbol under LD_PRELOAD) is freed
 * exactly as the reference frees it, the weighted-parsimony buffers included. NULL: nothing. */
void pll_parsimony_destroy(pll_parsimony_t *parsimony);
/* New. packedvector[node] and node_cost[node] are a lazily refreshed host mirror in the reference's layout: this
 * downloads one node (node < 0: all). Same contract as pll_gpu_sync_clv. For a weighted structure: sbuffer[node] and
 * anc_states[node] (see "weighted parsimony" below). */
int pll_gpu_sync_parsimony(pll_parsimony_t *parsimony, int node);
/* New. scores[i] = pll_fastparsimony_edge_score(parsimony, pairs[2i], pairs[2i+1]) for i < count: one launch (the pairs
 * on a grid axis) and one copy back. PLL_SUCCESS / PLL_FAILURE + pll_errno; nothing is written on failure. */
int pll_gpu_fastparsimony_edge_scores(const pll_parsimony_t *parsimony, const unsigned int *pairs, unsigned int count,
                                      unsigned int *scores);
/* New: all candidate edges of one stepwise-addition step at once. scores[i] = score of the tree that results from
 * inserting `node` into the edge whose two facing vectors are a = edges[2i], b = edges[2i+1]. With F(a,b) the Fitch
 * parent vector and U(x,y) the number of bit positions where no state is shared:
 *   scores[i] = cost[a] + cost[b] + cost[node] + U(a,b) + U(F(a,b), node) + const_cost
 * - exactly what the reference returns for pll_fastparsimony_update_vector({tmp, a, b}) followed by
 * pll_fastparsimony_edge_score(tmp, node) (src/stepwise.c:507-512). F(a,b) never leaves the registers, nothing is written
 * but the scores; one launch and one copy back for all edges. */
int pll_gpu_fastparsimony_insertion_scores(const pll_parsimony_t *parsimony, unsigned int node, const unsigned int *edges,
                                           unsigned int count, unsigned int *scores);
/* kernel launches of the last pll_fastparsimony_* / pll_gpu_fastparsimony_* call on the structure - or, for a weighted
 * structure, of the last pll_parsimony_build / score / reconstruct / pll_gpu_parsimony_insertion_scores call (the
 * transposing launch that carries stale mirrors up is not counted) */
unsigned int pll_gpu_fastparsimony_last_launch_count(const pll_parsimony_t *parsimony);
/* wait for everything enqueued on the structure's stream (either kind) */
int pll_gpu_synchronize_parsimony(pll_parsimony_t *parsimony);

/* ---- weighted (Sankoff) parsimony (src/pll.h:2535-2559; src/parsimony.c:24-67, :117-383) ----------------------------
 * The cost of a tree under a states x states matrix of substitution costs, and the ancestral characters that attain it
 * (examples/parsimony/npr-pars.c). Score buffers, ancestral buffers and the matrix live in HBM; the arithmetic is
 * binary64 add and min, every min over the same sums as in the reference, so every score buffer carries the reference's
 * bits. A fast-parsimony structure handed to one of these calls, or a weighted one handed to a pll_fastparsimony_* call,
 * is refused with PLL_ERROR_PARAM_INVALID.
 *
 * Failure convention (the reference has none): pll_errno is PLL_ERROR_PARAM_INVALID (a structure this library did not
 * create, a NULL argument, an index out of range - a score index must be < tips + score_buffers, an ancestral index in
 * [tips, tips + ancestral_buffers); the whole list is checked before anything is uploaded or launched),
 * PLL_ERROR_GPU_UNAVAILABLE (a host-only structure) or PLL_ERROR_GPU_RUNTIME. A score is then -INFINITY, a
 * reconstruction writes nothing.
 *
 * Mirror contract: sbuffer[i] is a lazily refreshed host mirror in the reference's [site][state] layout.
 * pll_set_parsimony_sequence writes it and marks it stale on the device; every stale buffer goes up before the next
 * launch, all of them in one copy. What a build computes stays on the device until pll_gpu_sync_parsimony(parsimony, i)
 * (i < 0: everything) downloads score buffer i and ancestral buffer i, or after every build under
 * PLL_AMD_EAGER_MIRROR=1 (the parents of the list; examples/parsimony/npr-pars.c:243 reads sbuffer raw). A caller that
 * writes sbuffer[i] itself says so with pll_gpu_parsimony_invalidate(parsimony, i): the host copy is then the newer one.
 * anc_states[] needs no sync after pll_parsimony_reconstruct.
 *
 * pll_parsimony_create (src/pll.h:2540, src/parsimony.c:117-202): the host fields are exactly the reference's - the
 * parameters, a private copy of the matrix, sbuffer[0 .. tips + score_buffers) of sites * states zeroed doubles,
 * anc_states[tips .. tips + ancestral_buffers) of `sites` zeroed words (entries below `tips` NULL), every
 * fast-parsimony field zero. Deliberate differences: states outside 1..64 (pll_state_t has 64 bits), tips == 0,
 * sites == 0 or a NULL matrix give NULL with PLL_ERROR_PARAM_INVALID. The structure owns a device record (all buffers,
 * the matrix, a stream of its own) in the side table of the fast structures. Under PLL_AMD_HOST_ONLY=1 the host fields
 * are filled and no device is touched; without a device and without that switch: NULL, PLL_ERROR_GPU_UNAVAILABLE. */
pll_parsimony_t *pll_parsimony_create(unsigned int tips, unsigned int states, unsigned int sites, const double *score_matrix,
                                      unsigned int score_buffers, unsigned int ancestral_buffers);
/* src/pll.h:2535, src/parsimony.c:24-67: entry j of a site is 0 where bit j of the mapped character is set and
 * `largest matrix entry + 1` elsewhere. A character that maps to 0: PLL_FAILURE, PLL_ERROR_TIPDATA_ILLEGALSTATE, the
 * reference's message in pll_errmsg and on stdout. tip_index >= tips + score_buffers: PLL_ERROR_PARAM_INVALID. */
int pll_set_parsimony_sequence(pll_parsimony_t *parsimony, unsigned int tip_index, const pll_state_t *map, const char *sequence);
/* src/pll.h:2547, src/parsimony.c:204-284. The result equals executing the list in order; dependency levels as for
 * pll_fastparsimony_update_vectors, every level ONE launch. Returns pll_parsimony_score of the last operation's parent.
 * Synchronous. count == 0 or a NULL list is refused. */
double pll_parsimony_build(pll_parsimony_t *parsimony, const pll_pars_buildop_t *operations, unsigned int count);
/* src/pll.h:2556, src/parsimony.c:286-307: the sum over the sites of the smallest entry. One launch and 8 bytes back; the
 * sum is formed in an order that depends on the site count alone (same bits from run to run; the reference adds site by
 * site, so the two agree to sites * 2^-52 relative, exactly where every term is an integer). */
double pll_parsimony_score(pll_parsimony_t *parsimony, unsigned int score_buffer_index);
/* src/pll.h:2551, src/parsimony.c:309-383, the reference's rule exactly: operation 0 gives its node the character of the
 * first minimal state; a later one keeps its parent's character where min + 1 > the parent's score at the parent's
 * character, and takes the character of its own first minimum otherwise. One launch per dependency level (an operation
 * depends on the earlier one that wrote its parent's ancestral buffer; a parent assigned by an earlier call is simply
 * read). anc_states[] of every node the list names is copied back before the call returns, in one copy. A map in which
 * some state has no single-bit character makes the reference index with the trailing-zero count of 0; here such a site
 * reads state 0 - its value is unspecified, nothing is read out of bounds. */
void pll_parsimony_reconstruct(pll_parsimony_t *parsimony, const pll_state_t *map, const pll_pars_recop_t *operations,
                               unsigned int count);
/* New. The caller has written sbuffer[index] directly: it goes up before the next launch. */
int pll_gpu_parsimony_invalidate(pll_parsimony_t *parsimony, unsigned int index);
/* New, the weighted twin of pll_gpu_fastparsimony_insertion_scores. scores[i] is BY DEFINITION what the reference returns
 * for pll_parsimony_build(parsimony, {{t1, edges[2i], edges[2i+1]}, {t2, t1, node}}, 2) with two spare buffers t1, t2.
 * No spare buffer is needed - both nodes live in registers and LDS - and nothing is written but the scores. One launch
 * for all candidates (long lists are cut: pllgpu_spars_insertion_scores in pll_amd_device.h) and one copy back. Every
 * scores[i] has the same bits alone, among others, in any list order and from run to run. PLL_SUCCESS, or PLL_FAILURE
 * with pll_errno and scores untouched. count == 0 succeeds without a launch. */
int pll_gpu_parsimony_insertion_scores(const pll_parsimony_t *parsimony, unsigned int node, const unsigned int *edges,
                                       unsigned int count, double *scores);

/* ---- the flat core seam of the hot path (src/pll.h:1049-1177 and :1295-1414; bodies in
 * src/core_partials.c:48-1210, src/core_likelihood.c:24-1496) ----------------------------------
 * Same signatures as the reference: raw HOST arrays in the layout `attrib` describes (PLL_ATTRIB_ARCH_*
 * -> states_padded; PLL_ATTRIB_RATE_SCALERS -> [entry][rate] scalers). Every call wraps its arrays in a
 * partition of the call's shape and runs the device path (csrc/host/core_seam.c): complete, but priced at a
 * PCIe round trip per call - use the partition-level functions above for speed. Small shapes are kept per
 * thread, shape and device for the next call (at most 32 MB each, 128 MB together, least recently used out
 * first; PLL_AMD_SEAM_CACHE=0: none); pll_core_seam_release() gives the calling thread's back at once.
 * The lookup table of pll_core_create_lookup is private to its pair with pll_core_update_partial_tt,
 * as in the reference (there: products per pair of tip states; here: the two matrices). */
void pll_core_seam_release(void); /* (no counterpart in the reference, whose core functions hold no state) */
void pll_core_create_lookup(unsigned int states, unsigned int rate_cats, double *lookup, const double *left_matrix,
                            const double *right_matrix, const pll_state_t *tipmap, unsigned int tipmap_size, unsigned int attrib);
void pll_core_create_lookup_4x4(unsigned int rate_cats, double *lookup, const double *left_matrix, const double *right_matrix);
void pll_core_update_partial_tt(unsigned int states, unsigned int sites, unsigned int rate_cats, double *parent_clv,
                                unsigned int *parent_scaler, const unsigned char *left_tipchars, const unsigned char *right_tipchars,
                                const pll_state_t *tipmap, unsigned int tipmap_size, const double *lookup, unsigned int attrib);
void pll_core_update_partial_tt_4x4(unsigned int sites, unsigned int rate_cats, double *parent_clv, unsigned int *parent_scaler,
                                    const unsigned char *left_tipchars, const unsigned char *right_tipchars, const double *lookup,
                                    unsigned int attrib);
void pll_core_update_partial_ti(unsigned int states, unsigned int sites, unsigned int rate_cats, double *parent_clv,
                                unsigned int *parent_scaler, const unsigned char *left_tipchars, const double *right_clv,
                                const double *left_matrix, const double *right_matrix, const unsigned int *right_scaler,
                                const pll_state_t *tipmap, unsigned int tipmap_size, unsigned int attrib);
void pll_core_update_partial_ti_4x4(unsigned int sites, unsigned int rate_cats, double *parent_clv, unsigned int *parent_scaler,
                                    const unsigned char *left_tipchars, const double *right_clv, const double *left_matrix,
                                    const double *right_matrix, const unsigned int *right_scaler, unsigned int attrib);
void pll_core_update_partial_ii(unsigned int states, unsigned int sites, unsigned int rate_cats, double *parent_clv,
                                unsigned int *parent_scaler, const double *left_clv, const double *right_clv,
                                const double *left_matrix, const double *right_matrix, const unsigned int *left_scaler,
                                const unsigned int *right_scaler, unsigned int attrib);
void pll_core_update_partial_repeats(unsigned int states, unsigned int parent_sites, unsigned int left_sites, unsigned int right_sites,
                                     unsigned int rate_cats, double *parent_clv, unsigned int *parent_scaler, const double *left_clv,
                                     const double *right_clv, const double *left_matrix, const double *right_matrix,
                                     const unsigned int *left_scaler, const unsigned int *right_scaler,
                                     const unsigned int *parent_id_site, const unsigned int *left_site_id,
                                     const unsigned int *right_site_id, double *bclv_buffer, unsigned int attrib);
void pll_core_update_partial_repeats_generic(unsigned int states, unsigned int parent_sites, unsigned int left_sites,
                                             unsigned int right_sites, unsigned int rate_cats, double *parent_clv,
                                             unsigned int *parent_scaler, const double *left_clv, const double *right_clv,
                                             const double *left_matrix, const double *right_matrix, const unsigned int *left_scaler,
                                             const unsigned int *right_scaler, const unsigned int *parent_id_site,
                                             const unsigned int *left_site_id, const unsigned int *right_site_id,
                                             double *bclv_buffer, unsigned int attrib);
void pll_core_update_partial_repeatsbclv_generic(unsigned int states, unsigned int parent_sites, unsigned int left_sites,
                                                 unsigned int right_sites, unsigned int rate_cats, double *parent_clv,
                                                 unsigned int *parent_scaler, const double *left_clv, const double *right_clv,
                                                 const double *left_matrix, const double *right_matrix,
                                                 const unsigned int *left_scaler, const unsigned int *right_scaler,
                                                 const unsigned int *parent_id_site, const unsigned int *left_site_id,
                                                 const unsigned int *right_site_id, double *bclv_buffer, unsigned int attrib);
double pll_core_edge_loglikelihood_ii(unsigned int states, unsigned int sites, unsigned int rate_cats, const double *parent_clv,
                                      const unsigned int *parent_scaler, const double *child_clv, const unsigned int *child_scaler,
                                      const double *pmatrix, double *const *frequencies, const double *rate_weights,
                                      const unsigned int *pattern_weights, const double *invar_proportion, const int *invar_indices,
                                      const unsigned int *freqs_indices, double *persite_lnl, unsigned int attrib);
double pll_core_edge_loglikelihood_ti(unsigned int states, unsigned int sites, unsigned int rate_cats, const double *parent_clv,
                                      const unsigned int *parent_scaler, const unsigned char *tipchars, const pll_state_t *tipmap,
                                      unsigned int tipmap_size, const double *pmatrix, double *const *frequencies,
                                      const double *rate_weights, const unsigned int *pattern_weights, const double *invar_proportion,
                                      const int *invar_indices, const unsigned int *freqs_indices, double *persite_lnl,
                                      unsigned int attrib);
double pll_core_edge_loglikelihood_ti_4x4(unsigned int sites, unsigned int rate_cats, const double *parent_clv,
                                          const unsigned int *parent_scaler, const unsigned char *tipchars, const double *pmatrix,
                                          double *const *frequencies, const double *rate_weights, const unsigned int *pattern_weights,
                                          const double *invar_proportion, const int *invar_indices, const unsigned int *freqs_indices,
                                          double *persite_lnl, unsigned int attrib);
double pll_core_edge_loglikelihood_repeats(unsigned int states, unsigned int sites, const unsigned int child_sites, unsigned int rate_cats,
                                           const double *parent_clv, const unsigned int *parent_scaler, const double *child_clv,
                                           const unsigned int *child_scaler, const double *pmatrix, double **frequencies,
                                           const double *rate_weights, const unsigned int *pattern_weights, const double *invar_proportion,
                                           const int *invar_indices, const unsigned int *freqs_indices, double *persite_lnl,
                                           const unsigned int *parent_site_id, const unsigned int *child_site_id, double *bclv,
                                           unsigned int attrib);
double pll_core_edge_loglikelihood_repeats_generic(unsigned int states, unsigned int sites, const unsigned int child_sites,
                                                   unsigned int rate_cats, const double *parent_clv, const unsigned int *parent_scaler,
                                                   const double *child_clv, const unsigned int *child_scaler, const double *pmatrix,
                                                   double **frequencies, const double *rate_weights, const unsigned int *pattern_weights,
                                                   const double *invar_proportion, const int *invar_indices,
                                                   const unsigned int *freqs_indices, double *persite_lnl,
                                                   const unsigned int *parent_site_id, const unsigned int *child_site_id, double *bclv,
                                                   unsigned int attrib);
double pll_core_root_loglikelihood(unsigned int states, unsigned int sites, unsigned int rate_cats, const double *clv,
                                   const unsigned int *scaler, double *const *frequencies, const double *rate_weights,
                                   const unsigned int *pattern_weights, const double *invar_proportion, const int *invar_indices,
                                   const unsigned int *freqs_indices, double *persite_lnl, unsigned int attrib);
double pll_core_root_loglikelihood_repeats(unsigned int states, unsigned int sites, unsigned int rate_cats, const double *clv,
                                           const unsigned int *site_id, const unsigned int *scaler, double *const *frequencies,
                                           const double *rate_weights, const unsigned int *pattern_weights,
                                           const double *invar_proportion, const int *invar_indices, const unsigned int *freqs_indices,
                                           double *persite_lnl, unsigned int attrib);

/* flat forms of the derivative path and of the transition matrices (src/pll.h:1181-1273, :2400-2412;
 * bodies src/core_derivatives.c:26-118, :219-320, :324-470, :474-640, :695-930 and src/core_pmatrix.c:186-247).
 * Same seam as above: raw host arrays in, a throw-away partition, the device path, the result copied
 * back - `sumtable` here is a real table in the reference's layout, not a handle. The model arrives per
 * rate category (eigenvecs[k], freqs[k], prop_invar[k]); pll_core_update_pmatrix indexes its arrays
 * through params_indices and pmatrix[] through matrix_indices, as the reference does.
 * pll_core_likelihood_derivatives refuses PLL_ATTRIB_AB_* (the correction needs the partition's extra
 * entries: pll_compute_likelihood_derivatives serves it). */
int pll_core_update_sumtable_ii(unsigned int states, unsigned int sites, unsigned int rate_cats, const double *parent_clv,
                                const double *child_clv, const unsigned int *parent_scaler, const unsigned int *child_scaler,
                                double *const *eigenvecs, double *const *inv_eigenvecs, double *const *freqs, double *sumtable,
                                unsigned int attrib);
int pll_core_update_sumtable_ti(unsigned int states, unsigned int sites, unsigned int rate_cats, const double *parent_clv,
                                const unsigned char *left_tipchars, const unsigned int *parent_scaler, double *const *eigenvecs,
                                double *const *inv_eigenvecs, double *const *freqs, const pll_state_t *tipmap,
                                unsigned int tipmap_size, double *sumtable, unsigned int attrib);
/* src/pll.h:1217-1226 */
int pll_core_update_sumtable_ti_4x4(unsigned int sites, unsigned int rate_cats, const double *parent_clv,
                                    const unsigned char *left_tipchars, const unsigned int *parent_scaler,
                                    double *const *eigenvecs, double *const *inv_eigenvecs, double *const *freqs,
                                    double *sumtable, unsigned int attrib);
/* src/core_likelihood.c:211-223 (exported there, not declared in src/pll.h): unpadded layout */
double pll_core_root_loglikelihood_repeats_generic(unsigned int states, unsigned int sites, unsigned int rate_cats,
                                                   const double *clv, const unsigned int *site_id, const unsigned int *scaler,
                                                   double *const *frequencies, const double *rate_weights,
                                                   const unsigned int *pattern_weights, const double *invar_proportion,
                                                   const int *invar_indices, const unsigned int *freqs_indices, double *persite_lnl);
int pll_core_update_sumtable_repeats(unsigned int states, unsigned int sites, unsigned int parent_sites, unsigned int rate_cats,
                                     const double *clvp, const double *clvc, const unsigned int *parent_scaler,
                                     const unsigned int *child_scaler, double *const *eigenvecs, double *const *inv_eigenvecs,
                                     double *const *freqs, double *sumtable, const unsigned int *parent_site_id,
                                     const unsigned int *child_site_id, double *bclv_buffer, unsigned int inv, unsigned int attrib);
int pll_core_update_sumtable_repeats_generic(unsigned int states, unsigned int sites, unsigned int parent_sites,
                                             unsigned int rate_cats, const double *clvp, const double *clvc,
                                             const unsigned int *parent_scaler, const unsigned int *child_scaler,
                                             double *const *eigenvecs, double *const *inv_eigenvecs, double *const *freqs,
                                             double *sumtable, const unsigned int *parent_site_id,
                                             const unsigned int *child_site_id, double *bclv_buffer, unsigned int inv,
                                             unsigned int attrib);
int pll_core_likelihood_derivatives(unsigned int states, unsigned int sites, unsigned int rate_cats, const double *rate_weights,
                                    const unsigned int *parent_scaler, const unsigned int *child_scaler, unsigned int parent_ids,
                                    unsigned int child_ids, const int *invariant, const unsigned int *pattern_weights,
                                    double branch_length, const double *prop_invar, double *const *freqs, const double *rates,
                                    double *const *eigenvals, const double *sumtable, double *d_f, double *dd_f,
                                    unsigned int attrib);
int pll_core_update_pmatrix(double **pmatrix, unsigned int states, unsigned int rate_cats, const double *rates,
                            const double *branch_lengths, const unsigned int *matrix_indices, const unsigned int *params_indices,
                            const double *prop_invar, double *const *eigenvals, double *const *eigenvecs,
                            double *const *inv_eigenvecs, unsigned int count, unsigned int attrib);

/* ---- branch-length derivatives (src/pll.h:834-852, src/derivatives.c:239-418; SURVEY section 8
 * row f1). `sumtable` is the caller's buffer of sites*rate_cats*states_padded doubles, as in the
 * reference, but it is used as a HANDLE: pll_update_sumtable computes the table into HBM and
 * remembers which host buffer it stands for; pll_compute_likelihood_derivatives given the same
 * pointer streams the device copy. The host buffer itself is only filled by
 * pll_gpu_sync_sumtable() (or under PLL_AMD_EAGER_MIRROR=1); a table the library has never seen
 * (written by the caller) is uploaded from the host buffer. Up to 16 tables per partition stay
 * resident (pll_gpu_release_sumtable). */
int pll_update_sumtable(pll_partition_t *partition, unsigned int parent_clv_index,
                        unsigned int child_clv_index, int parent_scaler_index,
                        int child_scaler_index, const unsigned int *params_indices, double *sumtable);
int pll_compute_likelihood_derivatives(pll_partition_t *partition, int parent_scaler_index,
                                       int child_scaler_index, double branch_length,
                                       const unsigned int *params_indices, const double *sumtable,
                                       double *d_f, double *dd_f);

/* ---- Newton branch-length optimisation in one call (this library's own; the reference ships only the bare
 * t -= d/dd loop of examples/newton/newton.c:55-92, one pll_compute_likelihood_derivatives per step). The whole
 * iteration runs on the device: one launch per derivative evaluation, chained without a host wait; the host polls
 * once per 8 evaluations. The first five arguments mean what they mean to pll_compute_likelihood_derivatives;
 * `sumtable` is the handle pll_update_sumtable filled (a recycled handle fails, a table the library has never seen
 * is uploaded). All arithmetic is binary64; d / dd are d_f / dd_f, the derivatives of -lnL:
 *
 *   t = clamp(t_start, t_min, t_max); lo = t_min; hi = t_max; lo_open = hi_open = true
 *   repeat up to max_iters times:
 *     (d, dd) = derivatives at t                          -- one row (t, d, dd) of the trace
 *     if |d| < tolerance: CONVERGED, stop
 *     if d > 0: if t == t_min: AT_MIN, stop;  hi = t; hi_open = false
 *     else:     if t == t_max: AT_MAX, stop;  lo = t; lo_open = false
 *     cand = dd > 0 ? t - d/dd : (d > 0 ? lo : 2*t)
 *     if !(cand > lo): cand = lo_open ? lo : 0.5*(lo+hi)    -- also a NaN
 *     else if !(cand < hi): cand = hi_open ? hi : 0.5*(lo+hi)
 *     if cand == t: STALLED, stop
 *     t = cand
 *   otherwise: MAXITER                                      -- result.t stays the last point evaluated
 *
 * (d_f, dd_f) of every row are bit for bit what pll_compute_likelihood_derivatives returns at that t on the same
 * table. |d| < tolerance is a statement about the slope, not about t: on a flat tail (a very long branch) it holds
 * at once. With matrix_index >= 0 the transition matrix of result.t is left in that slot exactly as
 * pll_update_prob_matrices(partition, params_indices, &matrix_index, &result.t, 1) would leave it (host mirror
 * through pll_gpu_sync_pmatrix), for every status, so pll_update_partials can follow with no further call.
 *
 * Fails with PLL_ERROR_PARAM_INVALID - before anything is flushed or launched - for a NULL partition,
 * params_indices, sumtable, options or result, !(0 <= t_min <= t_max) or non-finite t_min / t_max / t_start,
 * !(tolerance > 0), max_iters outside 1..PLL_GPU_NEWTON_MAX_ITERS, matrix_index < -1 or >= prob_matrices,
 * params_indices[k] >= rate_matrices; PLL_ERROR_GPU_UNAVAILABLE without a device; PLL_ERROR_GPU_UNSUPPORTED for the
 * Lewis and Felsenstein ascertainment-bias corrections (their correction is host arithmetic on separate terms after
 * every evaluation: use pll_compute_likelihood_derivatives; the Stamatakis correction is served, its extra entries
 * are ordinary weighted sites). On any failure *result and trace are untouched. Synchronous;
 * pll_gpu_last_launch_count reports the launches of the call. */
#define PLL_GPU_NEWTON_MAX_ITERS 64
#define PLL_GPU_NEWTON_CONVERGED 0   /* |d_f| < tolerance at result.t */
#define PLL_GPU_NEWTON_AT_MIN    1   /* t == t_min and d_f > 0 there */
#define PLL_GPU_NEWTON_AT_MAX    2   /* t == t_max and d_f < 0 there */
#define PLL_GPU_NEWTON_STALLED   3   /* the next point equals the current one (bracket exhausted) */
#define PLL_GPU_NEWTON_MAXITER   4   /* max_iters evaluations done, none of the above */

typedef struct pll_gpu_newton
{
  double t_start, t_min, t_max, tolerance;
  unsigned int max_iters;      /* 1 .. PLL_GPU_NEWTON_MAX_ITERS */
  int matrix_index;            /* >= 0: leave P(result.t) in this prob-matrix slot; -1: none */
} pll_gpu_newton_t;

typedef struct pll_gpu_newton_result
{
  double t, d_f, dd_f;         /* the last point evaluated and its derivatives; t is the answer */
  unsigned int iterations;     /* derivative evaluations performed */
  unsigned int host_waits;     /* times the call blocked on the device */
  int status;
} pll_gpu_newton_result_t;

int pll_gpu_optimize_branch_length(pll_partition_t *partition, int parent_scaler_index, int child_scaler_index,
                                   const unsigned int *params_indices, const double *sumtable,
                                   const pll_gpu_newton_t *options, pll_gpu_newton_result_t *result,
                                   double *trace /* NULL, or 3 * max_iters doubles: (t, d_f, dd_f) per evaluation */);

/* ---- site repeats bookkeeping (src/pll.h:682-742, src/repeats.c) --------------------------- */
/* scaler vector of a parent whose children are class-compressed (src/pll.h:727-742,
 * src/repeats.c:392-540): parent[i] = left[lids[site]] + right[rids[site]] with site = psites[i]; a NULL
 * map is the identity, a NULL scaler contributes 0. Integer utilities on host arrays, like
 * pll_fill_parent_scaler; the kernels fold this step into the update. */
void pll_fill_parent_scaler_repeats(unsigned int sites, unsigned int *parent_scaler, const unsigned int *psites,
                                    const unsigned int *left_scaler, const unsigned int *lids, const unsigned int *right_scaler,
                                    const unsigned int *rids);
void pll_fill_parent_scaler_repeats_per_rate(unsigned int sites, unsigned int rates, unsigned int *parent_scaler,
                                             const unsigned int *psites, const unsigned int *left_scaler, const unsigned int *lids,
                                             const unsigned int *right_scaler, const unsigned int *rids);
#define PLL_GET_ID(site_id, site) ((site_id) ? ((site_id)[(site)]) : (site))
#define PLL_GET_SITE(id_site, site) ((id_site) ? ((id_site)[(site)]) : (site))
int pll_repeats_enabled(const pll_partition_t *partition);
void pll_resize_repeats_lookup(pll_partition_t *partition, unsigned int size);
unsigned int pll_get_sites_number(const pll_partition_t *partition, unsigned int clv_index);
unsigned int *pll_get_site_id(const pll_partition_t *partition, unsigned int clv_index);
unsigned int *pll_get_id_site(const pll_partition_t *partition, unsigned int clv_index);
unsigned int pll_get_clv_size(const pll_partition_t *partition, unsigned int clv_index);
unsigned int pll_default_enable_repeats(pll_partition_t *partition, unsigned int left_clv,
                                        unsigned int right_clv);
unsigned int pll_no_enable_repeats(pll_partition_t *partition, unsigned int left_clv,
                                   unsigned int right_clv);
void pll_default_reallocate_repeats(pll_partition_t *partition, unsigned int parent,
                                    int scaler_index, unsigned int sites_to_alloc);
int pll_repeats_initialize(pll_partition_t *partition);
int pll_update_repeats_tips(pll_partition_t *partition, unsigned int tip_index,
                            const pll_state_t *map, const char *sequence);
void pll_update_repeats(pll_partition_t *partition, const pll_operation_t *op);
void pll_disable_bclv(pll_partition_t *partition);
void pll_fill_parent_scaler(unsigned int scaler_size, unsigned int *parent_scaler,
                            const unsigned int *left_scaler, const unsigned int *right_scaler);

/* ---- device-residency contract (new; SURVEY section 7 "hard parts" 1 and 2) ---------------- */
/* CLVs and scalers live in HBM; partition->clv[i] / scale_buffer[i] are a lazily refreshed host
 * mirror. Callers that read those arrays directly call one of these first. */
int pll_gpu_sync_clv(pll_partition_t *partition, unsigned int clv_index);     /* D2H one CLV */
int pll_gpu_sync_scaler(pll_partition_t *partition, unsigned int scaler_index);
/* transition matrices computed by pll_update_prob_matrices live on the device; this refreshes
 * partition->pmatrix[index] (index < 0: every matrix that is newer on the device) */
int pll_gpu_sync_pmatrix(pll_partition_t *partition, int index);
/* site-repeats class maps of inner nodes are computed on the device; pll_get_site_id() /
 * pll_get_id_site() refresh the host arrays they return, this call does it explicitly for callers
 * that read partition->repeats->pernode_* directly (node < 0: all nodes) */
int pll_gpu_sync_repeats(pll_partition_t *partition, int node);
int pll_gpu_sync_all(pll_partition_t *partition);
/* Callers that WRITE partition arrays directly (instead of through the setters above) tell the
 * library which device copies are stale. what = bitwise OR of PLL_GPU_DIRTY_*; index = array
 * slot or -1 for "all". */
#define PLL_GPU_DIRTY_PMATRIX 1u
#define PLL_GPU_DIRTY_FREQS 2u
#define PLL_GPU_DIRTY_RATE_WEIGHTS 4u
#define PLL_GPU_DIRTY_PATTERN_WEIGHTS 8u
#define PLL_GPU_DIRTY_INVARIANT 16u
#define PLL_GPU_DIRTY_CLV 32u    /* host copy of clv[index] is newer than the device copy */
#define PLL_GPU_DIRTY_SCALER 64u
#define PLL_GPU_DIRTY_TIPCHARS 128u
#define PLL_GPU_DIRTY_REPEATS 256u
#define PLL_GPU_DIRTY_EIGEN 512u /* eigenvecs / inv_eigenvecs / eigenvals / rates written directly */
/* Site repeats: pll_update_repeats / pll_update_partials keep, per node, what the class map standing on the device was
 * computed from (the two children, the versions of their maps, the lookup size) and launch nothing for an op whose
 * inputs have not moved - the maps are a function of the children's maps alone (src/repeats.c:299-382), so a
 * re-evaluation of the same tree after new branch lengths recomputes none and a topology move only the ancestors of
 * the moved edge. FORGET_REPEATS drops that knowledge for node `index` (-1: every node) without marking any host map
 * as newer: the next update computes the maps derived from it again (benchmarks of the recomputation itself; callers
 * that changed pernode_ids or a map behind the library's back use PLL_GPU_DIRTY_REPEATS, which implies it). */
#define PLL_GPU_FORGET_REPEATS 1024u
void pll_gpu_invalidate(pll_partition_t *partition, unsigned int what, int index);
/* download the device sumtable that stands for this host buffer into it (reference layout) */
int pll_gpu_sync_sumtable(pll_partition_t *partition, double *sumtable);
/* a partition keeps up to 16 device sumtables alive, one per host buffer handed to
 * pll_update_sumtable; beyond that the least recently used is recycled and an evaluation on ITS
 * handle fails with PLL_ERROR_GPU_RUNTIME (never a silent read of the unwritten host buffer). A
 * caller that is done with a table (about to free the host buffer) gives its HBM back here.
 * A recycled handle stays marked until pll_update_sumtable or this call names it again: a caller that frees an
 * evicted table and later fills a NEW buffer that malloc happened to place at the same address must announce it
 * (pll_gpu_release_sumtable(partition, buffer) before the first pll_compute_likelihood_derivatives on it) - otherwise
 * the evaluation fails with PLL_ERROR_GPU_RUNTIME instead of uploading the buffer. Resident tables are CLV-sized
 * (1M-site DNA: 128 MB each, up to 16 per partition): release what is no longer needed. */
int pll_gpu_release_sumtable(pll_partition_t *partition, const double *sumtable);
/* stream plumbing: by default each partition owns a stream; a harness may substitute its own
 * (a hipStream_t passed as void*) so that its events see the kernels. pll_update_partials is
 * asynchronous and may hold its last one or two operations back until the next call on the
 * partition (they are evaluated inside the edge log-likelihood kernel if that is the next call,
 * DESIGN.md "Tail fusion"); pll_gpu_synchronize(), pll_gpu_get_stream() and the timer calls launch
 * whatever is held, so a harness that brackets work with its own events calls one of them first. */
int pll_gpu_set_stream(pll_partition_t *partition, void *hip_stream);
void *pll_gpu_get_stream(const pll_partition_t *partition);
int pll_gpu_synchronize(pll_partition_t *partition);
/* Multi-GPU building block (SURVEY section 8 row e): pll_compute_edge_loglikelihood
 * (src/pll.h:790-797) without the host round trip. The evaluation is enqueued on the partition's
 * stream and leaves {lnL of this partition's sites, call sequence number} in the two doubles of
 * DEVICE memory at device_result; nothing is copied back and the call does not wait. A site-sharded
 * run hands device_result[0] of every rank to one RCCL all-reduce on the same stream
 * (pll_gpu_set_stream) and reads the sum once. Returns PLL_SUCCESS when enqueued. Not available
 * with an ascertainment-bias correction (its formula runs on the host). */
int pll_gpu_edge_loglikelihood_async(pll_partition_t *partition, unsigned int parent_clv_index,
                                     int parent_scaler_index, unsigned int child_clv_index,
                                     int child_scaler_index, unsigned int matrix_index,
                                     const unsigned int *freqs_indices, double *device_result);
/* ---- batched insertion log-likelihoods ---------------------------------
 * "What is the log-likelihood if the subtree is inserted into edge (child1, child2)?" for `count` candidate edges
 * in one call: the question an SPR move or a placement asks of tens to hundreds of edges. lnl[i] is the value the
 * reference returns for pll_update_partials with the one operation {tmp, tmp_scaler, child1..., child2...} of
 * candidate i (src/partials.c:237-291) followed by pll_compute_edge_loglikelihood(partition, tmp, tmp_scaler,
 * subtree_clv_index, subtree_scaler_index, subtree_matrix_index, freqs_indices, NULL) (src/likelihood.c:586-636),
 * with tmp a spare inner CLV and scaler. No such slot is needed: the inserted node's CLV and scaling counts exist
 * inside the kernel only, and nothing in the partition is written - no CLV, scaler, matrix or cached launch plan.
 * Any of the three ends may be an inner CLV (with or without a scaler), a PLL_ATTRIB_PATTERN_TIP tip or a tip set
 * through pll_set_tip_states; a scaler index named for a tip is ignored, as the reference's tip kernels do.
 * All candidates are read in one launch, so both ends of every candidate edge must hold the orientation the caller
 * means AT THE SAME TIME: a caller computes the "upward" CLV of each edge into a spare clv_buffers slot first
 * ("Scoring every regraft edge at once"). What the previous pll_update_partials still holds back
 * is launched first, so a candidate may name a node that traversal produces.
 * Synchronous; one copy back for all candidates. Each lnl[i] is formed in an order that depends on the site count
 * alone: it has the same bits whether the candidate is scored alone or among any others, and from run to run.
 * PLL_SUCCESS, or PLL_FAILURE with pll_errno and lnl untouched: PLL_ERROR_PARAM_INVALID for any index out of range
 * or a NULL argument with count > 0 (the whole list is checked before anything is flushed or launched);
 * PLL_ERROR_GPU_UNSUPPORTED for a PLL_ATTRIB_SITE_REPEATS partition (the inserted node has no class map) and for a
 * partition with an ascertainment-bias correction; PLL_ERROR_GPU_UNAVAILABLE without a device; count == 0 succeeds
 * without a launch. pll_gpu_last_launch_count reports the launches of the call. */
typedef struct pll_gpu_insertion
{
  unsigned int child1_clv_index;
  int child1_scaler_index;
  unsigned int child1_matrix_index;
  unsigned int child2_clv_index;
  int child2_scaler_index;
  unsigned int child2_matrix_index;
} pll_gpu_insertion_t;
int pll_gpu_insertion_loglikelihoods(pll_partition_t *partition, unsigned int subtree_clv_index, int subtree_scaler_index,
                                     unsigned int subtree_matrix_index, const pll_gpu_insertion_t *candidates,
                                     unsigned int count, const unsigned int *freqs_indices, double *lnl);
/* ---- batched NNI scores -------------------------------------------------
 * "What is the log-likelihood if the four subtrees around this inner edge are paired the other two ways?" for `count`
 * quartets in one call: the question a search that ranks the NNI neighbourhood of a tree asks of each of its T - 3 inner
 * edges. A quartet names its four ends e0..e3, each oriented towards the quartet's inner edge, with the matrix of each
 * end's own branch (it travels with the end) and the matrix of the inner edge. For quartet i the call returns
 *   lnl[3 i + 0] for ((e0,e1),(e2,e3)),  lnl[3 i + 1] for ((e0,e2),(e1,e3)),  lnl[3 i + 2] for ((e0,e3),(e1,e2)).
 * Arrangement ((x,y),(z,w)) is BY DEFINITION what the reference returns for pll_update_partials with the two operations
 * {tmp1, s1, x, matrix[x], scaler[x], y, matrix[y], scaler[y]} and {tmp2, s2, z, matrix[z], scaler[z], w, matrix[w],
 * scaler[w]} (src/partials.c:237-291), tmp1 / tmp2 spare inner CLVs with scalers s1 / s2, followed by
 * pll_compute_edge_loglikelihood(partition, tmp1, s1, tmp2, s2, inner_matrix_index, freqs_indices, NULL)
 * (src/likelihood.c:586-636): the child order inside a pair is the order written, the pair that holds e0 is the edge's
 * parent end, both nodes always scale, a pair of two tips follows the reference's tip-tip rule. No spare slot is
 * needed: both nodes and their scaling counts exist inside the kernel only, and nothing in the partition is written - no
 * CLV, scaler, matrix, class map or cached launch plan.
 * Any end may be an inner CLV (with or without a scaler), a PLL_ATTRIB_PATTERN_TIP tip or a tip set through
 * pll_set_tip_states; a scaler index named for a tip is ignored, as the reference's tip kernels do.
 * All four ends of every quartet are read in one launch, so each must hold the named orientation AT THE SAME TIME: a
 * caller computes the "upward" CLVs into spare clv_buffers slots first, exactly as for the insertion call
 * ("Scoring every NNI at once"). What the previous pll_update_partials still holds back is launched
 * first. For an inner edge p of a pll_utree, e0 = p->next->back, e1 = p->next->next->back, e2 = p->back->next->back,
 * e3 = p->back->next->next->back make arrangement 0 the tree itself, arrangement 2 the tree after the NNI that swaps
 * p->next with p->back->next and arrangement 1 the tree after the one that swaps p->next with p->back->next->next
 * ("Scoring every NNI at once", has the table).
 * Synchronous: one copy back and one wait. Each value is formed in an order that depends on the site count alone: it has
 * the same bits alone, among others, in any list order, and from run to run.
 * PLL_SUCCESS, or PLL_FAILURE with pll_errno, the usual line on stderr and lnl untouched. The whole list is checked
 * before anything is flushed or launched, in this order: PLL_ERROR_PARAM_INVALID for a NULL partition, for a NULL
 * quartets, lnl or freqs_indices with count > 0, for any index of any quartet or a freqs_indices[k] out of range;
 * PLL_ERROR_GPU_UNSUPPORTED for a PLL_ATTRIB_SITE_REPEATS partition and for a partition with an ascertainment-bias
 * correction; PLL_ERROR_GPU_UNAVAILABLE without a device. count == 0 succeeds without a launch and without touching
 * lnl. pll_gpu_last_launch_count reports the launches of the call; long lists are cut internally (the rule:
 * include/pll_amd_device.h, pllgpu_quartet_loglikelihoods).
 * Not offered: a choice of fewer than three arrangements, optimised branch lengths per arrangement, site repeats and the
 * ascertainment-bias correction (refused). */
typedef struct pll_gpu_quartet
{
  unsigned int clv_index[4];      /* the four ends e0..e3, each oriented towards the quartet's inner edge */
  int scaler_index[4];            /* PLL_SCALE_BUFFER_NONE or a scale buffer; ignored for a tip */
  unsigned int matrix_index[4];   /* the matrix of each end's own branch */
  unsigned int inner_matrix_index;
} pll_gpu_quartet_t;
int pll_gpu_quartet_loglikelihoods(pll_partition_t *partition, const pll_gpu_quartet_t *quartets, unsigned int count,
                                   const unsigned int *freqs_indices, double *lnl /* [count][3] */);
/* ---- branch supports: per-site and resampled quartet log-likelihoods ----
 * "How well supported is each inner branch?" - the SH-like aLRT and the RELL bootstrap need, for every inner edge, the
 * PER-SITE log-likelihoods of the tree and its two NNI neighbours and the sums of those under a few hundred to a few
 * thousand resampled site-weight vectors. One call gives both for `count` quartets. Quartets, arrangements a = 0, 1, 2 and
 * the tip-tip scaling rule are exactly those of pll_gpu_quartet_loglikelihoods; nothing in the partition is written (its
 * pattern weights included). With u_{i,a}[n] the log-likelihood of site n under arrangement a of quartet i BEFORE the
 * pattern weight:
 *   lnl[3 i + a]                              bit for bit what pll_gpu_quartet_loglikelihoods returns for the same list;
 *   persite[(3 i + a) * sites + n]            u_{i,a}[n] * pattern_weights[n]: the reference's persite_lnl[n] of that value's
 *                                             pll_compute_edge_loglikelihood (src/core_likelihood.c multiplies before it stores);
 *   resampled[(i * replicates + b) * 3 + a]   sum_n w_b[n] * u_{i,a}[n] with w_b = replicate_weights + b * sites: what the
 *                                             reference's per-edge path returns for the value after
 *                                             pll_set_pattern_weights(partition, w_b). The partition's own pattern weights do
 *                                             not enter: a replicate's weights replace them. Non-finite values follow IEEE
 *                                             arithmetic, as the reference's site_lk *= w does (a site of likelihood zero
 *                                             under weight zero gives NaN).
 * replicate_weights is [replicates][sites], row b one weight vector as pll_set_pattern_weights takes it; the rows are
 * uploaded once per call and converted on the device. Each of lnl, resampled, persite may be NULL - not all three;
 * replicates == 0 is allowed (no weights are read, resampled may be NULL: the per-site form of the existing call), and
 * with replicates > 0 both replicate_weights and resampled are required.
 * The sums are formed in binary64 in an order that depends on the site count alone: a resampled value has the same bits
 * whichever other quartets and replicate rows the call carries, in any order, and from run to run.
 * Turning lnl / resampled into an SH-aLRT or RELL percentage is a few lines on the caller's side and deliberately not
 * part of the library ("Branch supports after the search").
 * PLL_SUCCESS, or PLL_FAILURE with pll_errno, the usual line on stderr and all three outputs untouched. The checks, in
 * this order: PLL_ERROR_PARAM_INVALID for a NULL partition (count == 0 then succeeds without a launch and without
 * touching an output), for NULL quartets or freqs_indices, for replicates > 0 with NULL replicate_weights or resampled,
 * for three NULL outputs, for any index of any quartet or a freqs_indices[k] out of range; PLL_ERROR_GPU_UNSUPPORTED
 * for a PLL_ATTRIB_SITE_REPEATS partition and for one with an ascertainment-bias correction; PLL_ERROR_GPU_UNAVAILABLE
 * without a device. Synchronous. pll_gpu_last_launch_count reports the launches of the call (three when nothing is cut: the
 * quartet launch, the contraction, its reduction); long lists are cut internally (the rule and the one exception to
 * "untouched" - persite after a device error in a later chunk: include/pll_amd_device.h,
 * pllgpu_quartet_resampled_loglikelihoods).
 * Not offered: site repeats and the ascertainment-bias correction (refused). Replicates generated on the device:
 * pll_gpu_quartet_rell_loglikelihoods below; weights that stay on the device between calls are not needed with it. */
int pll_gpu_quartet_resampled_loglikelihoods(pll_partition_t *partition, const pll_gpu_quartet_t *quartets, unsigned int count,
                                             const unsigned int *freqs_indices,
                                             const unsigned int *replicate_weights /* [replicates][sites] */, unsigned int replicates,
                                             double *lnl /* [count][3] or NULL */, double *resampled /* [count][replicates][3] */,
                                             double *persite /* [count][3][sites] or NULL */);
/* diagnosis: stream-event times in ms of the last such call's first chunk - ms[0] what puts the weights in place (the
 * upload; the draw of pll_gpu_quartet_rell_loglikelihoods), ms[1] the quartet launch, ms[2] contraction + reduction
 * (tools/quartet_resample_probe.py, tools/quartet_rell_probe.py) */
int pll_gpu_resample_last_times(const pll_partition_t *partition, double *ms /* [3] */);
/* ---- RELL weights drawn on the device ------------------------------------
 * The replicate weights of a RELL or non-parametric bootstrap are random numbers: a caller need neither draw them on a
 * CPU core nor move them. With p = the partition's pattern weights, total = sum p and cdf[n] = p[0] + ... + p[n], replicate
 * b is `total` draws; draw j takes a 64-bit word x(seed, b, j) from a counter-based generator (Philox-4x32-10, key = the
 * two halves of seed, counter = (j >> 1, 0, b, "RELL"); an even j takes words 0-1, an odd j words 2-3), forms
 * r = floor(x * total / 2^64) and increments w_b[n] for the first n with cdf[n] > r. So a pattern of weight 0 is never
 * drawn, every row adds up to `total`, a pattern's probability is p[n] / total up to total / 2^64, and row b - b the
 * ABSOLUTE replicate number - depends on (seed, b, p) alone: not on how many rows a call asks for, how it is cut, or the
 * run. pllamd/rell.py restates the definition in integer arithmetic; the device equals it bit for bit. For that reason no
 * handle to weights kept on the device exists: a row is cheaper to draw again than to keep or to move.
 *
 * pll_gpu_draw_replicate_weights: rows [first_replicate, first_replicate + replicates) into weights [replicates][sites],
 * each a vector as pll_set_pattern_weights takes it (a standard bootstrap's rows). The checks, in this order:
 * PLL_ERROR_PARAM_INVALID for a NULL partition (replicates == 0 then succeeds without a launch), for NULL weights;
 * PLL_ERROR_GPU_UNSUPPORTED for a PLL_ATTRIB_SITE_REPEATS partition and for one with an ascertainment-bias correction (the
 * rows could not be fed to the call below); PLL_ERROR_GPU_UNAVAILABLE without a device; PLL_ERROR_PARAM_INVALID when the
 * pattern weights add up to 0 or to 2^32 or more (the sum is formed on the device; a row's words are 32 bits).
 *
 * pll_gpu_quartet_rell_loglikelihoods: pll_gpu_quartet_resampled_loglikelihoods with rows 0 .. replicates - 1 of `seed` in
 * place of replicate_weights - lnl, resampled and persite have the bits that call returns for those rows. replicate_weights
 * here is an OUTPUT: NULL, or [replicates][sites], the rows that were used. The partition's pattern weights are what is
 * resampled; after pll_set_pattern_weights the next call draws from the new weights.
 * PLL_SUCCESS, or PLL_FAILURE with pll_errno, the usual line on stderr and all outputs untouched. The checks, in this
 * order: PLL_ERROR_PARAM_INVALID for a NULL partition (count == 0 then succeeds without a launch and without touching an
 * output), for NULL quartets or freqs_indices, for replicates > 0 with NULL resampled, for lnl, resampled and persite all
 * NULL, for any index of any quartet or a freqs_indices[k] out of range; PLL_ERROR_GPU_UNSUPPORTED for a
 * PLL_ATTRIB_SITE_REPEATS partition and for one with an ascertainment-bias correction; PLL_ERROR_GPU_UNAVAILABLE without a
 * device; with replicates > 0, PLL_ERROR_PARAM_INVALID for pattern weights that add up to 0 or to 2^32 or more.
 * replicates == 0 is pll_gpu_quartet_resampled_loglikelihoods with replicates == 0. Synchronous. pll_gpu_last_launch_count:
 * four when nothing is cut (the draw, the quartet launch, the contraction, its reduction), one more when the pattern
 * weights have changed since the last draw (their prefix sums). Long lists are cut by the rule of
 * pll_gpu_quartet_resampled_loglikelihoods; the exception to "untouched" is its own - persite, and here replicate_weights,
 * may hold earlier chunks after a device error in a later chunk (include/pll_amd_device.h). */
int pll_gpu_draw_replicate_weights(pll_partition_t *partition, unsigned long long seed, unsigned int first_replicate,
                                   unsigned int replicates, unsigned int *weights /* [replicates][sites] */);
int pll_gpu_quartet_rell_loglikelihoods(pll_partition_t *partition, const pll_gpu_quartet_t *quartets, unsigned int count,
                                        const unsigned int *freqs_indices, unsigned long long seed, unsigned int replicates,
                                        double *lnl /* [count][3] or NULL */, double *resampled /* [count][replicates][3] */,
                                        double *persite /* [count][3][sites] or NULL */,
                                        unsigned int *replicate_weights /* out: [replicates][sites], or NULL */);
/* ---- the gradient of every branch at once --------------------------------
 * "What are the first and second derivatives of the log-likelihood with respect to this branch?" for `count` branches in
 * one call: what a simultaneous Newton or L-BFGS step on all 2T - 3 branches, HMC or variational inference over branch
 * lengths, or ranking the branches worth optimising asks. d_f[i], dd_f[i] are BY DEFINITION what the reference returns
 * for pll_update_sumtable(partition, parent_clv_index, child_clv_index, parent_scaler_index, child_scaler_index,
 * params_indices, tmp) (src/derivatives.c:239-324) followed by pll_compute_likelihood_derivatives(partition,
 * parent_scaler_index, child_scaler_index, branch_length, params_indices, tmp, &d_f, &dd_f) (src/derivatives.c:333-418,
 * src/core_derivatives.c:643-694, :696-849): the derivatives of -lnL. No table is needed and none is written: a table row
 * exists inside the kernel only, and nothing in the partition is written - no CLV, scaler, matrix, tip representation,
 * class map, resident sumtable or cached launch plan (the two contraction matrices behind pll_update_sumtable are
 * refreshed through the same bookkeeping, so a later pll_update_sumtable sees what it expects).
 * Per-site scaling: the scalers are not read - they cancel in L'/L, and the reference reads none. With
 * PLL_ATTRIB_RATE_SCALERS column k of a site is multiplied by 2^(-256 min(s_k - min_k s_k, PLL_SCALE_RATE_MAXDIFF)), s_k
 * the parent's count plus the child's, an absent scaler counting 0 (src/core_derivatives.c:420-460). With prop_invar > 0
 * the rate is rate / (1 - pinv), each category becomes c0 (1 - pinv) + pi[inv] pinv, c1 (1 - pinv), c2 (1 - pinv), and the
 * invariant term enters unscaled, exactly as in the reference (:676-686). Also served: pattern weights, a params_indices
 * entry per rate category with rate_matrices > 1, and an eigensystem marked invalid, which is computed first, as
 * pll_update_sumtable does here.
 * Either end may be an inner CLV (with or without a scaler), a PLL_ATTRIB_PATTERN_TIP tip, a tip set through
 * pll_set_tip_states (read as codes where the device holds codes) or a dense tip; the tip may be the parent or the child.
 * Two ends that the device both holds as codes are refused in every mode (the reference refuses that under
 * PLL_ATTRIB_PATTERN_TIP; pll_update_sumtable here makes one tip dense otherwise, but this call writes nothing, and no
 * tree of three or more taxa has such a branch).
 * Both ends of every branch are read in one launch, so each must hold the named orientation AT THE SAME TIME: a caller
 * computes the "upward" CLVs into spare clv_buffers slots first, exactly as for the insertion call ("The
 * gradient of every branch at once"). What the previous pll_update_partials still holds back is launched first and CLVs a
 * tree launch left pending are stored first: a branch may name a node that traversal produced. A branch may be named twice.
 * Synchronous: one copy back for all values and one wait. Each value is formed in an order that depends on the site count
 * alone: it has the same bits alone, among others, in any list order, and from run to run.
 * PLL_SUCCESS, or PLL_FAILURE with pll_errno, the usual line on stderr and d_f, dd_f untouched. The whole list is checked
 * before anything is flushed or launched, in this order: PLL_ERROR_PARAM_INVALID for a NULL partition, for a NULL
 * branches, params_indices or d_f with count > 0, for a CLV or scaler index out of range (a scaler below -1 included), for
 * a branch length that is negative or not finite, for a params_indices[k] >= rate_matrices and for two code-tip ends;
 * PLL_ERROR_GPU_UNSUPPORTED for a PLL_ATTRIB_SITE_REPEATS partition and for a partition with any ascertainment-bias
 * correction (the Stamatakis one included: one rule across the batched calls); PLL_ERROR_GPU_UNAVAILABLE without a
 * device. count == 0 succeeds without a launch and reads nothing of the list. dd_f may be NULL.
 * pll_gpu_last_launch_count reports the launches of the call; long lists are cut internally (the rule:
 * include/pll_amd_device.h, pllgpu_branch_derivatives).
 * Not offered: the log-likelihood itself, per-site values, any iteration (pll_gpu_optimize_branch_length serves one
 * branch), site repeats and the ascertainment-bias correction (refused). */
typedef struct pll_gpu_branch
{
  unsigned int parent_clv_index;
  int parent_scaler_index;      /* PLL_SCALE_BUFFER_NONE or a scale buffer; ignored for a tip */
  unsigned int child_clv_index;
  int child_scaler_index;
  double branch_length;
} pll_gpu_branch_t;
int pll_gpu_branch_derivatives(pll_partition_t *partition, const pll_gpu_branch_t *branches, unsigned int count,
                               const unsigned int *params_indices, double *d_f, double *dd_f /* may be NULL */);
/* ---- rate and alpha gradients: per-category branch derivatives ----------
 * The same launch keeping each rate category's share of a branch's d_f, and the contraction of those shares that is the
 * gradient of -lnL with respect to the category rates (FreeRate rates; through dr_k/dalpha the gamma shape alpha) and to a
 * common multiplier of all branch lengths (the per-partition scaler of a proportional-branch-length analysis). With the
 * reference's own quantities (src/core_derivatives.c:643-694, :757-772, :843-847) - per site n and category k,
 * (c0_k, c1_k, c2_k) the contraction of the site's table row with (e, l e, l^2 e) after the per-rate excess factor and
 * after the invariant-sites step (c1_k (1 - pinv)), lk0 = sum_k w_k c0_k the site's site_lk[0], pw the pattern weights:
 *   d_cat[i][k] = sum_n pw[n] * ( - w_k c1_k[n] / lk0[n] )        so that sum_k d_cat[i][k] = d_f[i] up to rounding
 *   d_rates[k]  = sum_i (t_i / r_k) * d_cat[i][k]                 added in list order i = 0 .. count-1
 *   d_scale     = sum_i  t_i * d_f[i]                             added in list order
 * t_i = branches[i].branch_length, r_k = the partition's category rate. The log-likelihood depends on r_k only through
 * the products r_k t_b / (1 - pinv) of the branches b, so d_rates[k] is d(-lnL)/dr_k and d_scale the derivative with
 * respect to a multiplier of all lengths at 1 - PROVIDED the list names every branch of the tree exactly once, each end
 * oriented towards its branch ("Gradients of rates, alpha and the branch-length scaler"). The call does
 * not check that: it contracts what it is given. d_rates is the derivative with the other rates and the weights held
 * fixed: no renormalisation of the mean rate is applied.
 * Everything else is pll_gpu_branch_derivatives': what the ends may be, the flush of held work and pending CLVs, nothing
 * in the partition written, synchronous with one copy back and one wait, the checks and their order, the refusals (site
 * repeats and any ascertainment-bias correction: PLL_ERROR_GPU_UNSUPPORTED; no device: PLL_ERROR_GPU_UNAVAILABLE), outputs
 * untouched on failure. Added among the first checks, after the NULL partition: count == 0 succeeds without a launch and
 * leaves every output untouched except d_rates[0..rate_cats) and d_scale, which are set to 0; PLL_ERROR_PARAM_INVALID
 * when every output is NULL; then the NULL list, the list checks and the two refusals as in pll_gpu_branch_derivatives;
 * then, for pll_gpu_rate_gradient with d_rates asked, PLL_ERROR_PARAM_INVALID for a category rate that is not > 0 and
 * finite (t / r is the chain rule; a rate of zero has a finite derivative that this formula does not give) - before the
 * device is asked for, so before anything is flushed or launched. The same call with d_rates NULL takes such a rate.
 * Bits: d_f and dd_f are bit for bit pll_gpu_branch_derivatives' for the same list; every d_cat value has the same bits
 * alone, among others, in any list order and from run to run; d_rates and d_scale are formed on the device from those
 * values, each product rounded and then added in list order - the bits of that loop written over the outputs of
 * pll_gpu_branch_category_derivatives.
 * pll_gpu_last_launch_count: one per cut of the list (the rule for R + 2 values per workgroup: include/pll_amd_device.h,
 * pllgpu_branch_category_derivatives), plus one when d_rates or d_scale is asked for. PLL_ERROR_GPU_UNSUPPORTED also
 * where a shape other than 4 states x 4 categories needs more than 152 KB of LDS (32 rate_cats (states + 32) bytes).
 * Not offered: second derivatives with respect to rates (cross-branch terms), any iteration or line search, site repeats,
 * ascertainment bias; sharded runs add d_rates / d_scale of the shards with pll_gpu_group_sum. */
int pll_gpu_branch_category_derivatives(pll_partition_t *partition, const pll_gpu_branch_t *branches, unsigned int count,
                                        const unsigned int *params_indices,
                                        double *d_cat /* [count][rate_cats] */,
                                        double *d_f /* [count] or NULL */, double *dd_f /* [count] or NULL */);
int pll_gpu_rate_gradient(pll_partition_t *partition, const pll_gpu_branch_t *branches, unsigned int count,
                          const unsigned int *params_indices,
                          double *d_rates /* [rate_cats] or NULL */, double *d_scale /* 1 or NULL */,
                          double *d_cat /* [count][rate_cats] or NULL */, double *d_f /* [count] or NULL */);
/* ---- the model gradient: dlnL/dQ, GTR rates and frequencies ----------
 * The gradient of -lnL with respect to the substitution parameters and the state frequencies from one device call over the
 * list that pll_gpu_branch_derivatives reads: both ends of every branch, oriented towards it. Notation for one partition:
 * U = inv_eigenvecs[m], U^-1 = eigenvecs[m], lam = eigenvals[m] (the reference forms P = U diag(exp(lam tau)) U^-1,
 * src/core_pmatrix.c:213-234, so Q_m = U diag(lam) U^-1); row b of the list has the parent end p, the child end c and the
 * length t_b - roles, tips, per-rate scalers and the excess factor f_k exactly as in pll_gpu_branch_derivatives; w_k, r_k,
 * pinv_k, m(k) = params_indices[k], the pattern weights pw[n]; L_n the site's site_lk[0] of
 * src/core_derivatives.c:676-686 (the invariant term included, after the excess factors); tau_bk = r_k t_b / (1 - pinv_k).
 *   A_i(n,k)     = sum_x pi_x p_x(n,k) U[x][i]            B_j(n,k) = sum_y U^-1[j][y] c_y(n,k)     (the row's two factors)
 *   H_bk[i][j]   = sum_n pw[n] * w_k (1 - pinv_k) f_k(n) A_i(n,k) B_j(n,k) / L_n
 *   Phi_bk[i][j] = tau e^{lam_j tau} * g((lam_i - lam_j) tau),   g(x) = expm1(x)/x, g(0) = 1    (so Phi_ii = tau e^{lam_i tau})
 *   W_m[i][j]    = sum_b (in list order) sum_{k: m(k)=m} Phi_bk[i][j] * H_bk[i][j]
 *   d_q[m][x][y] = - sum_ij U^-1[i][x] W_m[i][j] U[y][j]                                         = d(-lnL)/dQ_m[x][y]
 *   d_root[m][x] = - (1/pi_x) sum_{k: m(k)=m} sum_ij U^-1[i][x] U[x][j] e^{lam_j tau_0k} H_0k[i][j]   (branches[0] only)
 * d_q is the derivative of -lnL with respect to every entry of the rate matrix taken as independent, the per-category time
 * scaling included, each P_bk in the orientation the list gives it; it does not depend on the choice of eigenvectors. The
 * log-likelihood is multilinear in the P_bk, so for any parameter theta that keeps the model reversible
 *   d(-lnL)/dtheta = sum_xy d_q[m][x][y] dQ_m[x][y]/dtheta
 * PROVIDED the list names every branch of the tree exactly once, each end oriented towards its branch - the proviso of
 * pll_gpu_rate_gradient, and not checked here either. d_root is the explicit dependence of -lnL on pi through the root
 * sum, needed for the frequency gradient alone and taken at branches[0]: a change of pi moves the matrices out of
 * reversibility with the old pi, so for d_root / d_freqs the orientation of the rows counts - branches[0] is the edge whose
 * two ends point at each other (the root edge of the traversal) and every other row has the root-side end as its parent,
 * which is the list of INTEGRATION.md with the root edge moved to the front. d_subst cares neither which way a row points
 * (d_q itself does: a flipped row contributes its transpose) nor which row comes first. Phi is evaluated through expm1 in a form without
 * positive exponents: coinciding and nearly coinciding eigenvalues (JC69) never meet a divided difference.
 * pll_gpu_subst_gradient_from_dq applies the chain rule to the library's own parametrisation (src/models.c:182-256
 * without the square-root symmetrisation): s_p = subst_params[p] / subst_params[last], a_xy = s_xy pi_y (x != y), a_xx =
 * - sum_{y != x} a_xy, mean = 2 sum_{x<y} s_xy pi_x pi_y, Q = a / mean. d_subst[p] is the derivative with respect to
 * subst_params[m][p], the array as the caller set it, the division by the last entry applied (so sum_p subst_params[p]
 * d_subst[p] = 0); d_freqs[x] the derivative with respect to frequencies[m][x] with the other frequencies held fixed - no
 * renormalisation: the Q part through a and mean, plus d_root (a caller with normalised frequencies uses g_x - sum_y pi_y
 * g_y). A scalar host routine in closed form, O(states^2) in all; it needs no device and reads subst_params / frequencies
 * of the partition. PLL_ERROR_PARAM_INVALID for a NULL partition or d_q_m, for both outputs NULL, for a params_index out
 * of range, for a frequency of the set <= PLL_EIGEN_MINFREQ (the reference eliminates such states) and for
 * subst_params[last] <= 0. pll_gpu_subst_gradient is the device call followed by that routine for every rate matrix that
 * a category uses; an unused one gets zeros.
 * Everything else is pll_gpu_branch_category_derivatives': what the ends may be, the flush of held work and pending CLVs,
 * nothing in the partition written (an invalid eigensystem is computed first, as pll_update_sumtable does), synchronous
 * with one copy back and one wait, the checks and their order (d_q mandatory where d_f is there), the refusals
 * (PLL_ERROR_GPU_UNSUPPORTED for site repeats, any ascertainment-bias correction; PLL_ERROR_PARAM_INVALID for two code-tip
 * ends; no device: PLL_ERROR_GPU_UNAVAILABLE), outputs untouched on failure. count == 0 succeeds without a launch and sets
 * every output to zeros. Added: after the two refusals and before the device is asked for, PLL_ERROR_GPU_UNSUPPORTED when
 * d_root / d_freqs is asked while prop_invar of a used rate matrix is > 0 (that needs a per-state sum over the invariant
 * sites); d_q and d_subst are served with any pinv; then, for every output, the shape's need of LDS (below). pll_gpu_subst_gradient checks first of all, after the NULL partition,
 * count == 0 and both outputs NULL, what the chain rule asks of every used set. Shapes other than 4 states x 4 categories
 * whose two parked vectors exceed the LDS of a workgroup are PLL_ERROR_GPU_UNSUPPORTED (the rule:
 * include/pll_amd_device.h, pllgpu_qmatrix_gradient; 20 states x 4 and 61 x 2 fit, 61 x 4 does not).
 * Bits: every output has the same bits from run to run for the same partition and list; sums over sites are formed in an
 * order that depends on the shape alone, sums over branches in list order; no floating-point atomics.
 * pll_gpu_last_launch_count: three per cut of the list plus one (the rule: include/pll_amd_device.h).
 * Not offered: site repeats, ascertainment bias, the frequency gradient with pinv > 0, second derivatives, any optimiser,
 * non-reversible models; sharded runs add the shards' d_q with pll_gpu_group_sum. */
int pll_gpu_qmatrix_gradient(pll_partition_t *partition, const pll_gpu_branch_t *branches, unsigned int count,
                             const unsigned int *params_indices,
                             double *d_q    /* [rate_matrices][states][states] */,
                             double *d_root /* [rate_matrices][states] or NULL */);
int pll_gpu_subst_gradient_from_dq(const pll_partition_t *partition, unsigned int params_index,
                                   const double *d_q_m /* [states][states] */, const double *d_root_m /* [states] or NULL */,
                                   double *d_subst /* [states (states-1)/2] or NULL */, double *d_freqs /* [states] or NULL */);
int pll_gpu_subst_gradient(pll_partition_t *partition, const pll_gpu_branch_t *branches, unsigned int count,
                           const unsigned int *params_indices,
                           double *d_subst /* [rate_matrices][states (states-1)/2] or NULL */,
                           double *d_freqs /* [rate_matrices][states] or NULL */);
/* ---- maximum-likelihood distances between tips --------------------------
 * The input of every distance method (NJ / BIONJ starting and guide trees, pre-filters for placement, saturation checks):
 * for every two tips of a list the branch length that maximises the likelihood of the two sequences alone, under the
 * partition's own model - in one call, without a CLV, a sumtable or a launch per evaluation.
 * For x = tips[i], y = tips[j], i < j: distance[i][j] is the t at which the safeguarded Newton recipe of
 * pll_gpu_optimize_branch_length (above; restated in pllamd/newton.py) stops when it is applied to the function that
 * pll_update_sumtable(partition, x, y, PLL_SCALE_BUFFER_NONE, PLL_SCALE_BUFFER_NONE, params_indices, ..) followed by
 * pll_compute_likelihood_derivatives evaluates, with x in the left role (contraction matrix 1) and y in the right; the same
 * t_start, t_min, t_max, tolerance and max_iters for every pair; options->matrix_index must be -1. d_f / dd_f are the
 * derivatives of -lnL at the returned distance (the last point evaluated), status one of PLL_GPU_NEWTON_*, iterations the
 * derivative evaluations performed. [i][j] and [j][i] of every array receive the same bits from one computation, diagonal
 * entries are 0, and a tip that appears twice makes an ordinary pair (AT_MIN, or CONVERGED on a flat function).
 * p_distance: with n_ab the summed pattern weight of the sites where the pair shows the codes (a, b), the sum of n_ab over
 * the code pairs whose state sets are disjoint, divided by the sum over the code pairs in which neither code is the
 * all-states set; 0 where that denominator is 0. Two integer sums and one division.
 * How: a site's sumtable row depends on its pair of codes alone, so the alignment enters only through n_ab. A workgroup
 * counts one pair's n_ab in one pass over the two code rows and runs the whole iteration on that table; nothing is
 * written to device memory but the answers. A pair's bits depend on its own two code rows, the model and the options
 * alone - not on the list, the position in it or how the list is cut into launches.
 * Every tip must be given by codes: a PLL_ATTRIB_PATTERN_TIP tip, or a tip set through pll_set_tip_states / an indicator
 * pll_set_tip_clv that the device holds as codes. Nothing in the partition is written (an invalid eigensystem is computed
 * first, as pll_update_sumtable does); what pll_update_partials holds back is launched first. Synchronous: one copy back,
 * one wait. pll_gpu_last_launch_count reports the launches (the rule: include/pll_amd_device.h, pllgpu_pairwise_distances).
 * PLL_SUCCESS, or PLL_FAILURE with pll_errno, the usual line on stderr and every output untouched. Everything is refused
 * before anything is flushed or launched, in this order: PLL_ERROR_PARAM_INVALID for a NULL partition, out or
 * out->distance; with count > 0 for a NULL tips, params_indices or options, a tips[i] >= tips, the option checks of
 * pll_gpu_optimize_branch_length, matrix_index != -1, a params_indices[k] >= rate_matrices, a tip not given by codes (a
 * dense pll_set_tip_clv tip, a partition without tip codes); PLL_ERROR_GPU_UNSUPPORTED for PLL_ATTRIB_SITE_REPEATS and
 * ascertainment-bias partitions, for prop_invar > 0 of a used rate matrix (the invariant-site term is a property of the
 * alignment column, not of the code pair), for a device code table beyond the limit (at most PLLGPU_DISTANCE_MAX_CODES =
 * 128 codes and the LDS rule of include/pll_amd_device.h: 16 codes for 4 states, one per distinct state set otherwise -
 * a 61-state alignment with ambiguity codes has about 64) and for pattern weights that add up to 2^32 or more;
 * PLL_ERROR_GPU_UNAVAILABLE without a device. count == 0 succeeds at once (after the first check; nothing else is read,
 * nothing written); count == 1 passes every check and succeeds without a launch, its one diagonal entry set to 0.
 * Not offered: invariant sites, site repeats, ascertainment bias, distances that involve inner nodes. */
typedef struct pll_gpu_distances
{
  double *distance;          /* [count*count], required: D[x*count+y], symmetric, 0 on the diagonal */
  double *p_distance;        /* NULL or [count*count] */
  double *d_f, *dd_f;        /* NULL or [count*count]: derivatives of -lnL at the returned distance */
  int *status;               /* NULL or [count*count]: PLL_GPU_NEWTON_* */
  unsigned int *iterations;  /* NULL or [count*count]: derivative evaluations performed */
} pll_gpu_distances_t;

int pll_gpu_pairwise_distances(pll_partition_t *partition, const unsigned int *tips, unsigned int count,
                               const unsigned int *params_indices, const pll_gpu_newton_t *options,
                               const pll_gpu_distances_t *out);

/* ---- neighbour-joining and BIONJ trees from distances ------------------------------------
 * The starting or guide tree of a distance matrix, joined on the device: pll_gpu_nj_tree from a matrix the caller holds,
 * pll_gpu_distance_tree from the tips of a partition - pll_gpu_pairwise_distances and the join in one call, the matrix
 * staying on the device unless distances_out asks for it. flags: 0 = NJ (Saitou & Nei 1987 in the form of Studier & Keppler
 * 1988), PLL_GPU_NJ_BIONJ = BIONJ (Gascuel 1997).
 * The tree: the tips are the nodes 0 .. count-1 in input order, the inner node made by join s (s = 0, 1, ...) is count + s,
 * and the last inner node, 2 count - 3, joins the three nodes that remain. parent[v] is the label of v's parent, length[v]
 * the branch to it; parent[2 count - 3] = -1 and length[2 count - 3] = 0. Lengths are what the algorithm gives: negative
 * ones are neither clamped nor flagged.
 * The definition is pllamd/nj.py, a numpy restatement usable without a device, which the kernels follow operation for
 * operation (every product rounded before it is added). With r active nodes, r > 3, and the row sums R_i = sum_k d_ik:
 *   Q_ij = (r-2) d_ij - (R_i + R_j);   the pair of minimal Q is joined, i the node with the smaller label;
 *   l_i = d_ij / 2 + (R_i - R_j) / (2 (r-2)),   l_j = d_ij - l_i;
 *   NJ:    d_uk = ((d_ik + d_jk) - d_ij) / 2,   R_u = ((R_i + R_j) - r d_ij) / 2;
 *   BIONJ: V starts as D; lambda = 1/2 + sum_{k != i,j} (V_jk - V_ik) / (2 (r-2) V_ij), clamped to [0, 1], 1/2 where
 *          V_ij = 0; d_uk = lambda (d_ik - l_i) + (1 - lambda) (d_jk - l_j), evaluated as
 *          (d_jk - l_j) + lambda ((d_ik - l_i) - (d_jk - l_j)): exact where the two sides agree (an additive matrix);
 *          V_uk = (lambda V_ik + (1 - lambda) V_jk) - lambda (1 - lambda) V_ij;
 *          R_u = B + lambda (A - B), A = (R_i - d_ij) - (r-2) l_i, B = (R_j - d_ij) - (r-2) l_j;
 *   the row sums are carried forward: R_k <- ((R_k - d_ik) - d_jk) + d_uk;
 *   three nodes a, b, c: l_a = ((d_ab + d_ac) - d_bc) / 2, and likewise for b and c.
 * Two rules make the answer a function of the input alone. Ties: among equal minimal Q the pair whose (smaller label,
 * larger label) comes first lexicographically. Four nodes left: Q_ab = Q_cd holds for every split, so only the three pairs
 * that contain the active node with the smallest label are searched.
 * How: two launches per join on one stream with no host wait between joins (the rule: include/pll_amd_device.h,
 * pllgpu_nj_tree); pll_gpu_nj_last_launch_count reports those of the calling thread's last pll_gpu_nj_tree,
 * pll_gpu_last_launch_count(partition) those of pll_gpu_distance_tree, distances and join together.
 * pll_gpu_nj_tree needs no partition: it owns a stream on `device` (-1: PLL_AMD_DEVICE, else the thread's current device)
 * for the length of the call, as pll_compress_site_patterns does. Working set on the device: 8 count^2 bytes, twice that for
 * BIONJ.
 * PLL_SUCCESS, or PLL_FAILURE with pll_errno, the usual line on stderr and parent, length and distances_out untouched.
 * pll_gpu_nj_tree refuses, before anything is launched, with PLL_ERROR_PARAM_INVALID: a NULL distances, parent or length;
 * count < 3; unknown flag bits; an entry [x][y], x < y, that is negative or not finite (one pass on the host);
 * PLL_ERROR_GPU_UNAVAILABLE without a device; PLL_ERROR_MEM_ALLOC when the device has no room.
 * pll_gpu_distance_tree makes every check of pll_gpu_pairwise_distances in its order (parent and length in the place of
 * out), then PLL_ERROR_PARAM_INVALID for count < 3 and unknown flag bits.
 * Not offered: row-minimum caches (RapidNJ), single precision, relaxed NJ. */
#define PLL_GPU_NJ_BIONJ 1u
int pll_gpu_nj_tree(const double *distances /* [count][count]; only [x][y], x < y, is read */, unsigned int count,
                    unsigned int flags, int device, int *parent /* [2 count - 2] */, double *length /* [2 count - 2] */);
int pll_gpu_distance_tree(pll_partition_t *partition, const unsigned int *tips, unsigned int count,
                          const unsigned int *params_indices, const pll_gpu_newton_t *options, unsigned int flags,
                          int *parent, double *length, double *distances_out /* NULL or [count][count] */);
unsigned int pll_gpu_nj_last_launch_count(void);
/* milliseconds between the first and the last launch of the calling thread's last join, measured by device events on the
 * stream it ran on (without the copies up and back); -1 if none ran */
double pll_gpu_nj_last_device_ms(void);

/* ---- bootstrap trees from distances ------------------------------------------------------
 * Felsenstein's bootstrap of the distance tree - hundreds to thousands of replicate trees of one alignment - without a
 * host loop: all replicates have the same count, so their joins run in lockstep, one search / join launch pair serving
 * step s of every one of them, and the distance kernel reads the alignment through one row of weights, so it is given
 * many. Turning the trees into split supports or a consensus is the caller's.
 *
 * pll_gpu_nj_trees: `replicates` matrices in one call. Tree b - parent + b (2 count - 2), length + b (2 count - 2) - has
 * bit for bit what pll_gpu_nj_tree gives on matrix b (distances + b count^2): its tree format, flags, tie rule and
 * four-node rule, and pllamd/nj.py's bits on exact inputs. The launches do not depend on `replicates` as long as the
 * matrices and working sets fit one chunk (the rule and the byte budget: include/pll_amd_device.h, pllgpu_nj_trees);
 * pll_gpu_nj_last_launch_count reports chunks x (2 (count - 3) + 2), chunks x 1 at count == 3. It owns a stream and its
 * blocks on `device` for the length of the call, as pll_gpu_nj_tree does.
 * Refused before anything is launched, with every output untouched: PLL_ERROR_PARAM_INVALID for a NULL distances, parent
 * or length, count < 3, unknown flag bits, or an entry [x][y], x < y, of any matrix that is negative or not finite;
 * PLL_ERROR_GPU_UNAVAILABLE without a device; PLL_ERROR_MEM_ALLOC when the device has no room. replicates == 0 succeeds
 * at once after the NULL, count and flag checks and writes nothing.
 *
 * pll_gpu_bootstrap_distance_trees: row b of every output is, bit for bit, what this sequence returns:
 *   1. row first_replicate + b of pll_gpu_draw_replicate_weights(partition, seed, ...) - the absolute numbering of that
 *      call: a call for rows 3..7 gives rows 3..7 of a call for rows 0..7;
 *   2. pll_set_pattern_weights with that row;
 *   3. pll_gpu_distance_tree(partition, tips, count, params_indices, options, flags, ...), out->distances its
 *      distances_out and out->status the status array of pll_gpu_pairwise_distances;
 * which is the composition of the definitions in pllamd/rell.py, pllamd/distances.py and pllamd/nj.py. But the partition's
 * pattern weights are not written, and neither is anything else it holds - CLVs, scalers, matrices, the resampling state
 * of other calls: the rows are drawn on the device where the distance kernel reads them and leave it only through
 * out->weights. Per chunk of replicates (the cut, the byte budget and the launch rule: include/pll_amd_device.h,
 * pllgpu_bootstrap_distance_trees) one draw launch, the distance launches, the joins and one wait;
 * pll_gpu_last_launch_count reports the launches.
 * PLL_SUCCESS, or PLL_FAILURE with pll_errno and the usual line on stderr. Refused before anything is flushed or launched,
 * with every output untouched, in this order: PLL_ERROR_PARAM_INVALID for a NULL partition, out, out->parent or
 * out->length; every check of pll_gpu_distance_tree, in its order; PLL_ERROR_PARAM_INVALID for pattern weights that add
 * up to 0 (the refusal of pll_gpu_draw_replicate_weights). replicates == 0 succeeds after the first check and writes
 * nothing. A device error after the checks may leave the rows of earlier chunks written.
 * Not offered: split supports or a consensus of the trees; several pairs or replicates per workgroup; rows of weights
 * supplied by the caller; site repeats, ascertainment bias and prop_invar > 0 (refused by the distance checks). */
typedef struct pll_gpu_bootstrap_trees
{
  int *parent;            /* [replicates][2 count - 2], required */
  double *length;         /* [replicates][2 count - 2], required */
  double *distances;      /* NULL or [replicates][count][count] */
  int *status;            /* NULL or [replicates][count][count]: PLL_GPU_NEWTON_* of every pair */
  unsigned int *weights;  /* NULL or [replicates][sites]: the rows drawn */
} pll_gpu_bootstrap_trees_t;

int pll_gpu_nj_trees(const double *distances /* [replicates][count][count]; only [x][y], x < y, is read */,
                     unsigned int count, unsigned int replicates, unsigned int flags, int device,
                     int *parent /* [replicates][2 count - 2] */, double *length /* [replicates][2 count - 2] */);
int pll_gpu_bootstrap_distance_trees(pll_partition_t *partition, const unsigned int *tips, unsigned int count,
                                     const unsigned int *params_indices, const pll_gpu_newton_t *options,
                                     unsigned int flags, unsigned long long seed, unsigned int first_replicate,
                                     unsigned int replicates, const pll_gpu_bootstrap_trees_t *out);
/* diagnosis (tools/bootstrap_trees_timing.py): device-event times of the last pll_gpu_bootstrap_distance_trees' first
 * chunk, in ms - ms[0] the draw, ms[1] the distance launches, ms[2] the joins */
int pll_gpu_bootstrap_last_times(const pll_partition_t *partition, double *ms);

/* ---- rate-category posteriors, site rates and EM weight steps ----------
 * The per-category site likelihoods of one edge - what every evaluation kernel mixes away in registers - and what model
 * optimisation makes of them: FreeRate (+R) and mixture (LG4X) weights, empirical-Bayes site rates, a pinv step. The
 * seven edge arguments are those of pll_compute_edge_loglikelihood. With w the category weights, pi_f(k) / p_f(k) the
 * frequency set and prop_invar of category k, r the category rates and pw the pattern weights:
 *   l[n][k] = sum_j pi_f(k)[j] x_k[n][j] (P_k y_k[n])[j]
 *   s[n][k] = the scaling counts of both ends added: per site (the same for every k), or per rate (PLL_ATTRIB_RATE_SCALERS)
 *   c[n]    = min_k s[n][k]            u[n][k] = l[n][k] * 2^(-256 min(s[n][k] - c[n], 4))    (what the edge kernels mix)
 *   A[n][k] = w_k (1 - p_f(k)) u[n][k]
 *   I[n][k] = w_k p_f(k) pi_f(k)[inv_n] if p_f(k) > 0 and site n is invariant, else 0
 * and, where c[n] > 0 and sum_k I > 0, A multiplied by 2^(-256 min(c[n], 4)) (src/core_likelihood.c:1156-1174);
 * L[n] = sum_k (A + I). Each output may be NULL (not all five); host layouts are site-major:
 *   cat_lnl[n][k]   = log(l[n][k]) - 256 ln2 * s[n][k]      exact: no cap at 4, no weight, no pinv, no pattern weight; -inf where l = 0
 *   posterior[n][k] = (A[n][k] + I[n][k]) / L[n]            rows sum to 1
 *   site_rates[n]   = sum_k (A[n][k] / L[n]) * r_k          the invariant share has rate 0
 *   weight_sums[k]  = sum_n pw[n] * posterior[n][k]         the EM numerator
 *   lnl             = sum_n pw[n] * site lnL                what pll_compute_edge_loglikelihood returns
 * A site with L[n] = 0 gets a zero posterior row and rate, adds nothing to weight_sums and makes lnl -inf.
 * The ends are oriented exactly as pll_compute_edge_loglikelihood orients them. What the previous pll_update_partials
 * still holds back is launched first and pending CLVs are stored first: an edge may name what a traversal produced.
 * Nothing in the partition is written. Synchronous: one copy back per output asked for and one wait; every sum is
 * formed in an order that depends on the site count alone. pll_gpu_last_launch_count: 1 with cat_lnl alone, 2 with
 * posterior or site_rates, 3 with weight_sums or lnl.
 * PLL_SUCCESS, or PLL_FAILURE with pll_errno, the usual line on stderr and every output untouched. The checks, all before
 * anything is launched or written, in this order: PLL_ERROR_PARAM_INVALID for a NULL partition, a NULL freqs_indices or
 * five NULL outputs; PLL_ERROR_PARAM_INVALID for an index out of range (a scaler below -1 included), a freqs_indices[k]
 * >= rate_matrices or two PLL_ATTRIB_PATTERN_TIP tip ends; PLL_ERROR_GPU_UNSUPPORTED for a PLL_ATTRIB_SITE_REPEATS
 * partition and for one with an ascertainment-bias correction; PLL_ERROR_GPU_UNAVAILABLE without a device. */
int pll_gpu_edge_category_posteriors(pll_partition_t *partition, unsigned int parent_clv_index, int parent_scaler_index,
                                     unsigned int child_clv_index, int child_scaler_index, unsigned int matrix_index,
                                     const unsigned int *freqs_indices, double *cat_lnl /* [sites][rate_cats] or NULL */,
                                     double *posterior /* [sites][rate_cats] or NULL */, double *site_rates /* [sites] or NULL */,
                                     double *weight_sums /* [rate_cats] or NULL */, double *lnl /* 1 or NULL */);
/* EM steps on the category weights over the same edge, in one call: the CLVs are read once, every step is a stream over
 * sites x rate_cats doubles on the device. Row 0 of weights_out is the start - start_weights, or the partition's
 * rate_weights for NULL - row i + 1 is S_k / (S_0 + ... + S_{R-1}), added in that order, with S = weight_sums evaluated
 * under row i, and lnl_out[i] (lnl_out may be NULL) is lnl under row i. steps == 0 is one evaluation. The partition's own
 * weights are neither read after row 0 is formed nor written: the caller hands the row it wants to
 * pll_set_category_weights. pll_gpu_last_launch_count: 1 + 2 (steps + 1), with no host wait between the launches.
 * The checks and their order are those above, with, among the first: NULL weights_out, steps > PLL_GPU_EM_MAX_STEPS, a
 * start weight that is negative or not finite, or start weights summing to 0 (PLL_ERROR_PARAM_INVALID). */
#define PLL_GPU_EM_MAX_STEPS 1024
int pll_gpu_category_weights_em(pll_partition_t *partition, unsigned int parent_clv_index, int parent_scaler_index,
                                unsigned int child_clv_index, int child_scaler_index, unsigned int matrix_index,
                                const unsigned int *freqs_indices, const double *start_weights /* [rate_cats] or NULL */,
                                unsigned int steps, double *weights_out /* [steps + 1][rate_cats] */,
                                double *lnl_out /* [steps + 1] or NULL */);
/* ---- batched placement log-likelihoods ---------------------------------
 * Every query x every candidate edge in one call: the pre-scoring pass of a phylogenetic placement, the first pass of
 * a stepwise addition by likelihood. lnl is [query_count][count], query-major, and lnl[q * count + i] is BY DEFINITION
 * what pll_gpu_insertion_loglikelihoods(partition, query_tip_indices[q], PLL_SCALE_BUFFER_NONE, pendant_matrix_index,
 * &candidates[i], 1, freqs_indices, ...) returns, bit for bit: the reference's pll_update_partials with the one
 * operation {tmp, tmp_scaler, child1..., child2...} of candidate i (src/partials.c:237-291) followed by
 * pll_compute_edge_loglikelihood(partition, tmp, tmp_scaler, query_tip_indices[q], PLL_SCALE_BUFFER_NONE,
 * pendant_matrix_index, freqs_indices, NULL) (src/likelihood.c:586-636). A caller may pre-score with this call and
 * score the best edges again with the other: the ranking does not move. The tree, its CLVs and the candidates are read
 * once per chunk of queries instead of once per query (a 4 x 4 candidate: about 264 + Q bytes per site, not 265 Q).
 * Queries are tips of the partition set through pll_set_tip_states, with or without PLL_ATTRIB_PATTERN_TIP; a caller
 * with more queries than spare tips sets the spare tips again chunk by chunk ("Scoring many queries at
 * once"). A tip may be named twice (two equal rows) and may also be an end of a candidate. Candidates are exactly those
 * of pll_gpu_insertion_loglikelihoods. Nothing in the partition is written - no CLV, scaler, matrix, class map or
 * cached launch plan; what the previous pll_update_partials still holds back is launched first. Synchronous: one copy
 * back of the whole matrix and one wait. Every lnl[q][i] has the same bits whatever else the two lists hold, in
 * whatever order, and from run to run.
 * PLL_SUCCESS, or PLL_FAILURE with pll_errno, the usual line on stderr and lnl untouched. Both lists are checked whole
 * before anything is flushed or launched, in this order: PLL_ERROR_PARAM_INVALID for a NULL partition, for a NULL
 * query_tip_indices, candidates, lnl or freqs_indices with both counts > 0, for a query index >= partition->tips, for a
 * pendant matrix, a candidate field or a freqs_indices[k] out of range; PLL_ERROR_GPU_UNSUPPORTED for a
 * PLL_ATTRIB_SITE_REPEATS partition, for a partition with an ascertainment-bias correction, and for a query tip the
 * device does not hold as codes (set with pll_set_tip_clv to anything but indicator vectors, made dense by an earlier
 * call, or PLL_AMD_NO_TIP_CODES on a partition without PLL_ATTRIB_PATTERN_TIP: set it again with pll_set_tip_states);
 * PLL_ERROR_GPU_UNAVAILABLE without a
 * device. query_count == 0 or count == 0 succeeds without a launch and without touching lnl.
 * pll_gpu_last_launch_count reports the launches of the call; long lists are cut internally by candidates and by
 * chunks of queries (the rule: include/pll_amd_device.h, pllgpu_placement_loglikelihoods).
 * Not offered: a pendant length per query (one matrix serves all), inner subtree ends as queries (the call above serves
 * one), site repeats and the ascertainment-bias correction (refused), the best k edges chosen on the device, and an
 * optimised pendant branch per placement (absent). */
int pll_gpu_placement_loglikelihoods(pll_partition_t *partition, const unsigned int *query_tip_indices,
                                     unsigned int query_count, unsigned int pendant_matrix_index,
                                     const pll_gpu_insertion_t *candidates, unsigned int count,
                                     const unsigned int *freqs_indices, double *lnl);
/* pll_compute_node_ancestral (src/pll.h:799-806) without the host round trip: the kernel is enqueued on the
 * partition's stream (pll_gpu_set_stream / pll_gpu_get_stream apply) and leaves the table in the sites * states
 * doubles of DEVICE memory at device_ancestral; nothing is copied back and the call does not wait. A caller that
 * reconstructs every inner node queues partial traversals and these calls on one stream and synchronises once.
 * Returns PLL_SUCCESS when enqueued. */
int pll_gpu_node_ancestral_async(pll_partition_t *partition, unsigned int node_clv_index, int node_scaler_index,
                                 unsigned int other_clv_index, int other_scaler_index, unsigned int matrix_index,
                                 const unsigned int *freqs_indices, void *device_ancestral);
/* ---- the ONE exchange of a site-sharded run (SURVEY section 8 row e) --------------------------
 * Sites are independent through every CLV update; the only cross-site operation of the path is the sum
 * of the per-site log-likelihoods (src/core_likelihood.c:1489, the sequential `logl += site_lk`). A run
 * that gives every GPU its own partition over a contiguous site range therefore needs exactly one
 * exchange per evaluation: the sum of one double per rank. Two forms, both plain C:
 *
 * (1) ranks of ONE node, fixed order - pll_gpu_group_*. The ranks (processes or threads) meet in a named
 *     POSIX shared-memory segment with two alternating slots per rank; every rank leaves {value, step}
 *     in its slot and adds the slots of all ranks IN RANK ORDER, so every rank returns the same bits and
 *     the sum is reproducible run to run whatever the arrival order (an all-reduce tree is not). Cost:
 *     a cache-line hand-off between host cores behind the result the device has already written to host
 *     memory - no kernel, no collective library. `name` must be unique per run and start with '/'.
 * (2) any communicator - pll_gpu_allreduce_lnl / pll_gpu_edge_loglikelihood_allreduce: one
 *     ncclAllReduce(sum, ncclDouble) on the partition's stream. librccl is opened with dlopen() at the
 *     first call (PLL_AMD_RCCL_LIB overrides the name), so the library loads and works without RCCL;
 *     the caller creates the ncclComm_t (ncclCommInitRank) and passes it as void *. */
typedef struct pll_gpu_group pll_gpu_group_t;
/* join (and, whoever comes first, create) the segment `name` as rank `rank` of `size`; waits until all
 * `size` ranks have joined (timeout_ms <= 0: 60 s). NULL + pll_errno on failure. */
pll_gpu_group_t *pll_gpu_group_join(const char *name, unsigned int rank, unsigned int size, int timeout_ms);
void pll_gpu_group_leave(pll_gpu_group_t *group);
unsigned int pll_gpu_group_rank(const pll_gpu_group_t *group);
unsigned int pll_gpu_group_size(const pll_gpu_group_t *group);
/* global[i] = local[i] of rank 0 + rank 1 + ... + rank size-1, in that order, i < count <= 6. Every
 * rank must call it the same number of times. PLL_FAILURE (pll_errno PLL_ERROR_GPU_RUNTIME) when a rank
 * does not arrive within the group's timeout. */
int pll_gpu_group_sum(pll_gpu_group_t *group, const double *local, unsigned int count, double *global);
/* pll_compute_edge_loglikelihood (src/pll.h:790-797) on this rank's partition followed by the exchange:
 * the log-likelihood of the WHOLE alignment on every rank (-inf on every rank if any rank failed).
 * persite_lnl, if given, receives this rank's sites only (per-site values stay sharded). */
double pll_gpu_group_edge_loglikelihood(pll_partition_t *partition, pll_gpu_group_t *group,
                                        unsigned int parent_clv_index, int parent_scaler_index,
                                        unsigned int child_clv_index, int child_scaler_index,
                                        unsigned int matrix_index, const unsigned int *freqs_indices,
                                        double *persite_lnl);
/* pll_compute_likelihood_derivatives (src/pll.h:2400-2412 region; src/derivatives.c:296-418) on this rank's partition
 * followed by the exchange of {d_f, dd_f}: the derivatives of the WHOLE alignment's log-likelihood on every rank,
 * the same bits everywhere (rank order), so that all ranks of a sharded branch-length optimisation take the same
 * Newton step. Every rank calls it with the same branch length. PLL_FAILURE on every rank if any rank failed
 * (that rank keeps its own pll_errno). group == NULL: the plain evaluation. */
int pll_gpu_group_likelihood_derivatives(pll_partition_t *partition, pll_gpu_group_t *group,
                                         int parent_scaler_index, int child_scaler_index, double branch_length,
                                         const unsigned int *params_indices, const double *sumtable,
                                         double *d_f, double *dd_f);
/* enqueue ncclAllReduce(device_values, device_values, count, ncclDouble, ncclSum, comm) on the
 * partition's stream (count doubles of DEVICE memory, e.g. what pll_gpu_edge_loglikelihood_async left) */
int pll_gpu_allreduce_lnl(pll_partition_t *partition, void *nccl_comm, double *device_values, unsigned int count);
/* set-up of a (partition, communicator) pair, once: binds librccl, asks ncclCommCount, reserves the 16-byte operand
 * in device memory. Everything that can fail before a collective is enqueued fails HERE - call it on every rank
 * after creating the communicator and agree on the results before the first collective evaluation
 * (pll_gpu_edge_loglikelihood_allreduce calls it itself when it meets a new communicator, but a rank that fails
 * there has not joined the collective its peers are in). PLL_SUCCESS / PLL_FAILURE + pll_errno. */
int pll_gpu_allreduce_prepare(pll_partition_t *partition, void *nccl_comm);
/* the whole step without a host round trip before the exchange: the shard's log-likelihood stays in
 * device memory, is all-reduced there and only the sum comes back. Collective: every rank of the
 * communicator calls it, the same number of times. Returns the sum, -inf on failure. Once the pair is
 * prepared, a rank whose own evaluation fails still takes part (its operand is -inf): every rank returns
 * -inf - that rank with its own pll_errno, the others with PLL_ERROR_GPU_RUNTIME - and nobody is left
 * waiting inside the collective for a rank that merely failed to evaluate. A rank that never calls (it died,
 * or returned from a failed set-up) cannot be helped by the callers that did: their all-reduce never completes;
 * they get -inf + PLL_ERROR_GPU_RUNTIME after PLL_AMD_REDUCE_TIMEOUT_MS (default 60 000) instead of blocking
 * for ever, with the partition's stream still stuck behind the collective - fatal for the job, but reported. */
double pll_gpu_edge_loglikelihood_allreduce(pll_partition_t *partition, void *nccl_comm,
                                            unsigned int parent_clv_index, int parent_scaler_index,
                                            unsigned int child_clv_index, int child_scaler_index,
                                            unsigned int matrix_index, const unsigned int *freqs_indices);
/* 1 if a RCCL library could be opened (pll_gpu_allreduce_* usable), 0 otherwise */
int pll_gpu_rccl_available(void);
/* HIP-event stopwatch on the partition's stream (bench.py's roofline leg): start .. stop
 * brackets whatever was enqueued in between; returns elapsed milliseconds from stop(). */
int pll_gpu_timer_start(pll_partition_t *partition);
double pll_gpu_timer_stop(pll_partition_t *partition);
/* number of kernel launches issued by the last pll_update_partials, pll_gpu_insertion_loglikelihoods,
 * pll_gpu_placement_loglikelihoods, pll_gpu_quartet_loglikelihoods or pll_gpu_branch_derivatives call */
unsigned int pll_gpu_last_launch_count(const pll_partition_t *partition);
/* site repeats: class-map operations computed on the device (launches = 0) / class kernels launched (launches != 0)
 * since the partition was created. An unchanged tree adds nothing, a topology move the ops of its partial traversal.
 * launches = 2: the class-map calls the device has served - one per pll_update_partials that had maps to compute, one
 * per dependency level with work under PLL_AMD_REP_LEVEL_SYNC=1 or a caller's enable_repeats; a call that runs its
 * levels a second time because its level forecast was wrong counts once */
unsigned long long pll_gpu_class_map_work(const pll_partition_t *partition, int launches);
/* pll_update_partials calls whose launches came from a plan the partition's device context had kept, since it was
 * created. A context's plans depend on ITS device blocks only: other partitions coming, growing and going leave them */
unsigned long long pll_gpu_plan_replays(const pll_partition_t *partition);
/* 1 if the last pll_update_partials call found its operation list, and everything its classification rests on, as the
 * call before left them and went straight to the launches (a re-evaluation of one tree); 0 if it took the whole path */
int pll_gpu_last_update_replayed(const pll_partition_t *partition);
/* HBM bytes the kernels of the last pll_update_partials call had to move by construction: child
 * reads + parent and scaler writes of every launch AS IT WAS GROUPED (an op evaluated together with
 * the producers of its children does not read those children back) - bench.py's roofline numerator */
double pll_gpu_last_algorithmic_bytes(const pll_partition_t *partition);
/* CLVs (with their scalers) that the last step computed and has not stored on the device: the 32 tip x tip parents of a
 * balanced 64-taxon DNA traversal evaluated together with its root edge as one launch (PLL_AMD_LAZY_CHERRIES=0: always 0) -
 * or, from the second step on of a loop that reads no CLV between its steps, all 56 CLVs of its eight 8-tip subtrees, levels
 * 1 to 3 (PLL_AMD_LAZY_SUBTREES=0: never more than 32; unset: for 20 000 entries and more).
 * Every call that reads one of them, overwrites it or changes its tip codes stores them first, in one launch; the same
 * traversal again simply recomputes them, and a change of a matrix they read leaves them pending (they keep the old one).
 * Nothing a caller has to do - the number says why a read launched something */
unsigned int pll_gpu_pending_clvs(const pll_partition_t *partition);
int pll_gpu_device_count(void);
/* 1 if a usable gfx950 device is present, 0 otherwise (the analogue of src/hardware.c's probe) */
int pll_gpu_available(void);

#ifdef __cplusplus
}
#endif
#endif /* PLL_AMD_H_ */
