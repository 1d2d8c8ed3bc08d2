/*
 * pll_amd_device.h - the thin C ABI between the C host code (libpll-2_amd/csrc/host) and the
 * HIP translation unit (libpll-2_amd/csrc/hip/pllgpu.hip) that owns the gfx950 kernels.
 *
 * Plain C: opaque context handle, indices, pointers and sizes only. The host side keeps every
 * libpll-2 semantic (pll_partition_t bookkeeping, op classification, dependency levels, site
 * repeats, error convention); this layer only moves bytes and launches kernels. Each entry point
 * names the reference routine whose arithmetic it replaces.
 *
 * All functions return 0 on success or a negative pllgpu_status; pllgpu_last_error() gives text.
 */
#ifndef PLL_AMD_DEVICE_H_
#define PLL_AMD_DEVICE_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pllgpu_ctx pllgpu_ctx_t;

enum pllgpu_status
{
  PLLGPU_OK = 0,
  PLLGPU_ENODEVICE = -1, /* no gfx950 device / HIP runtime unusable */
  PLLGPU_ENOMEM = -2,
  PLLGPU_ERUNTIME = -3,  /* a HIP call failed */
  PLLGPU_EINVAL = -4,
  PLLGPU_EUNSUPPORTED = -5
};

/* shape of one partition (immutable for the life of the context) */
typedef struct pllgpu_geometry
{
  unsigned int tips;
  unsigned int nodes;          /* tips + clv_buffers */
  unsigned int states;
  unsigned int states_padded;  /* host stride, kept on the device: mirror copies are memcpy */
  unsigned int rate_cats;
  unsigned int sites;          /* alignment sites */
  unsigned int sites_alloc;    /* sites + asc-bias extra sites */
  unsigned int prob_matrices;
  unsigned int rate_matrices;
  unsigned int scale_buffers;
  unsigned int per_rate_scalers; /* PLL_ATTRIB_RATE_SCALERS */
  unsigned int pattern_tip;      /* PLL_ATTRIB_PATTERN_TIP */
} pllgpu_geometry_t;

/* one CLV update after host-side classification (src/partials.c:24-235) */
#define PLLGPU_OP_LEFT_TIP 1u   /* left child is given by tip codes, not a CLV */
#define PLLGPU_OP_RIGHT_TIP 2u
#define PLLGPU_OP_GATHER 4u     /* at least one of the three nodes is class-compressed */
typedef struct pllgpu_op
{
  unsigned int parent_clv, left_clv, right_clv;       /* node indices */
  int parent_scaler, left_scaler, right_scaler;       /* scale buffer indices or -1 */
  unsigned int left_matrix, right_matrix;
  unsigned int parent_entries;                        /* sites, or class count under repeats */
  unsigned int flags;
  unsigned int level;                                 /* dependency level, 0-based */
  int war_level;                                      /* latest level at which an EARLIER op of the list still
                                                         reads or writes this op's parent CLV / scaler
                                                         (-1: none): the op may not run before it */
} pllgpu_op_t;

typedef struct pllgpu_edge
{
  unsigned int parent_clv, child_clv; /* parent is always a CLV node; child may be a tip */
  int parent_scaler, child_scaler;
  unsigned int matrix;
  unsigned int child_is_tip;
  unsigned int gather;                /* either end class-compressed */
  const unsigned int *freqs_indices;  /* host, [rate_cats] */
  int want_persite;
  double *device_result;              /* NULL: synchronous call. Otherwise 2 doubles of DEVICE memory:
                                         the kernel leaves {lnL, call sequence number} there and the
                                         call returns without waiting (multi-GPU: the sum over shards
                                         is reduced on the device, pll_gpu_edge_loglikelihood_async) */
  double sequence;                    /* 0: the context numbers the call itself. Otherwise the sequence word the
                                         kernel leaves next to the value (ranks of a collective number their
                                         evaluations in step, so that the reduced word identifies the step) */
} pllgpu_edge_t;

int pllgpu_device_count(void);
/* the device a context created now with device = -1 would live on (PLL_AMD_DEVICE=<n>, else the calling thread's
 * current HIP device); -2: any of them in turn (PLL_AMD_DEVICE=auto); and the device a context does live on */
/* site repeats, since the context was created: class-map ops handed to the device (launches = 0) or class kernels
 * launched (launches = 1) - what the version stamps of repeats.c save is visible here; launches = 2: the
 * pllgpu_repeats_classes calls served (non-empty lists that passed the checks; a call that runs its levels a second
 * time because its level forecast was wrong counts once) */
unsigned long long pllgpu_class_map_work(const pllgpu_ctx_t *ctx, int launches);
/* op lists launched from a plan the context had kept (the same list over blocks that have not moved), ever */
unsigned long long pllgpu_plan_replays(const pllgpu_ctx_t *ctx);
int pllgpu_default_device(void);
int pllgpu_context_device(const pllgpu_ctx_t *ctx);
const char *pllgpu_last_error(void);

pllgpu_ctx_t *pllgpu_create(const pllgpu_geometry_t *geo, int device);
void pllgpu_destroy(pllgpu_ctx_t *ctx);

/* ---- data movement ------------------------------------------------------------------------ */
/* entries = number of site entries (each entry is rate_cats*states_padded doubles) */
int pllgpu_clv_reserve(pllgpu_ctx_t *ctx, unsigned int node, unsigned int entries);
int pllgpu_clv_upload(pllgpu_ctx_t *ctx, unsigned int node, const double *host, unsigned int entries);
int pllgpu_clv_download(pllgpu_ctx_t *ctx, unsigned int node, double *host, unsigned int entries);
int pllgpu_scaler_reserve(pllgpu_ctx_t *ctx, unsigned int index, unsigned int entries);
int pllgpu_scaler_upload(pllgpu_ctx_t *ctx, unsigned int index, const unsigned int *host,
                         unsigned int entries);
int pllgpu_scaler_download(pllgpu_ctx_t *ctx, unsigned int index, unsigned int *host,
                           unsigned int entries);
/* on = 1: CLV and scaler downloads of up to 2 MB are enqueued and return before their bytes have arrived; on = 0: one
 * wait for all of them, after which every `host` buffer handed over since holds its data (a caller that wants a CLV and
 * its scaler vector pays one wait instead of two). Larger downloads wait as always. */
int pllgpu_download_defer(pllgpu_ctx_t *ctx, int on);
int pllgpu_tipchars_upload(pllgpu_ctx_t *ctx, unsigned int tip, const unsigned char *host,
                           unsigned int count);
/* code -> state mask table; NULL selects "code is the mask" (4-state, src/pll.c:875-910) */
int pllgpu_tipmap_upload(pllgpu_ctx_t *ctx, const unsigned long long *host, unsigned int count);
/* host_block: count matrices in the reference layout [rate][row][states_padded], contiguous
 * (src/pll.c:593-611); re-laid-out for the kernels during the upload */
int pllgpu_pmatrix_upload(pllgpu_ctx_t *ctx, unsigned int first, unsigned int count,
                          const double *host_block);
int pllgpu_frequencies_upload(pllgpu_ctx_t *ctx, unsigned int index, const double *host);
int pllgpu_rate_weights_upload(pllgpu_ctx_t *ctx, const double *host);
int pllgpu_prop_invar_upload(pllgpu_ctx_t *ctx, const double *host);
int pllgpu_pattern_weights_upload(pllgpu_ctx_t *ctx, const unsigned int *host, unsigned int count);
int pllgpu_invariant_upload(pllgpu_ctx_t *ctx, const int *host /* or NULL */, unsigned int count);
/* site repeats maps of one node (src/pll.h:292-297): site_id[sites_alloc] site -> class,
 * id_site[ids] class -> representative site; ids == 0 clears (node not compressed) */
int pllgpu_repeats_upload(pllgpu_ctx_t *ctx, unsigned int node, const unsigned int *site_id,
                          const unsigned int *id_site, unsigned int ids);

/* ---- compute ------------------------------------------------------------------------------ */
/* class maps computed ON the device (replaces the table walk of
 * pll_update_repeats, src/repeats.c:299-382, and - for ops with force == 0 - the decision of
 * pll_default_enable_repeats, src/repeats.c:100-110): for every op the parent's site -> class and
 * class -> first-site maps from the children's maps. The ops of a whole traversal go in ONE call,
 * sorted by dependency level (ops of one level are mutually independent): a child produced by an
 * earlier op of the call is named by that op's index (lsrc / rsrc), its class count is taken from
 * device memory; a child from outside the call (lsrc / rsrc = -1) must have its maps on the device,
 * nleft / nright are its class counts (0: not compressed). force = 1: the host has decided to
 * compress this parent (a caller-supplied enable_repeats callback), both children from outside.
 * lookup_size = pll_repeats_t::lookup_buffer_size. counts_out[i] = PLLGPU_REPEATS_COMPRESSED |
 * classes of ops[i].parent, or 0 where the rule said no. Synchronises once, at the end. */
#define PLLGPU_REPEATS_COMPRESSED 0x80000000u
#define PLLGPU_REPEATS_MAX_OPS 65536u
typedef struct pllgpu_repop
{
  unsigned int parent, left, right;
  unsigned int nleft, nright;
  int lsrc, rsrc;
  unsigned int level;
  unsigned int force;
} pllgpu_repop_t;
int pllgpu_repeats_classes(pllgpu_ctx_t *ctx, const pllgpu_repop_t *ops, unsigned int count,
                           unsigned int lookup_size, unsigned int *counts_out);
/* how many classes the kernels shall assume for `node` (0 = one entry per site, maps unused) */
int pllgpu_repeats_set_ids(pllgpu_ctx_t *ctx, unsigned int node, unsigned int ids);
/* device maps of `node` back to the host: site_id[sites], id_site[ids]. Synchronises. */
int pllgpu_repeats_download(pllgpu_ctx_t *ctx, unsigned int node, unsigned int *site_id,
                            unsigned int *id_site, unsigned int ids);

/* replaces pll_core_update_partial_{ii,ti,tt,repeats} + pll_core_create_lookup
 * (src/core_partials.c:48-1210). Asynchronous on the context's stream. ops must be sorted by
 * level; ops of one level are independent. */
int pllgpu_update_partials(pllgpu_ctx_t *ctx, const pllgpu_op_t *ops, unsigned int count);
/* replaces pll_core_edge_loglikelihood_{ii,ti,ti_4x4,repeats} (src/core_likelihood.c:351-1496).
 * Synchronises. persite_host may be NULL. */
int pllgpu_edge_loglikelihood(pllgpu_ctx_t *ctx, const pllgpu_edge_t *edge, double *persite_host,
                              double *lnl_out);
/* replaces pll_core_root_loglikelihood[_repeats] (src/core_likelihood.c:25-349) */
int pllgpu_root_loglikelihood(pllgpu_ctx_t *ctx, unsigned int clv, int scaler, unsigned int gather,
                              const unsigned int *freqs_indices, double *persite_host,
                              double *lnl_out);

/* replaces, for `count` candidate edges at once, the pair pll_update_partials with one op into a spare node
 * (src/partials.c:237-291) + pll_compute_edge_loglikelihood between that node and the subtree end
 * (src/likelihood.c:586-636): host_out[i] = the log-likelihood with the subtree inserted into candidate i. The inserted
 * node exists in registers / LDS only (kernels_insertion.h); nothing the context holds is written. Any of the three
 * ends may be a tip given by codes (*_is_tip; its scaler index is not read). Every index of the whole list is checked
 * before held work is launched or anything else happens; class-compressed CLVs anywhere in the context and
 * ascertainment-bias entries are PLLGPU_EUNSUPPORTED. One launch per kInsMaxCands candidates (counted into
 * pllgpu_last_launch_count), one copy back, one wait; host_out is written only on success. */
typedef struct pllgpu_insertion
{
  unsigned int child1_clv;
  int child1_scaler;
  unsigned int child1_matrix;
  unsigned int child2_clv;
  int child2_scaler;
  unsigned int child2_matrix;
  unsigned int child1_is_tip, child2_is_tip;
} pllgpu_insertion_t;
int pllgpu_insertion_loglikelihoods(pllgpu_ctx_t *ctx, unsigned int subtree_clv, int subtree_scaler, unsigned int subtree_matrix,
                                    unsigned int subtree_is_tip, const pllgpu_insertion_t *cands, unsigned int count,
                                    const unsigned int *freqs_indices, double *host_out);

/* The same question for `queries` query tips at once: host_out[q * count + i] = what pllgpu_insertion_loglikelihoods gives
 * for the subtree end (query_tips[q], no scaler, pendant_matrix, a tip given by codes) and candidate i, bit for bit. The
 * inserted node of a candidate is formed once per site tile and a chunk of queries is scored against it
 * (kernels_placement.h). Every query must be a tip whose codes the context holds (PLLGPU_EINVAL otherwise). Every index
 * of both lists is checked before held work is launched or anything else happens; class-compressed CLVs anywhere in the
 * context and ascertainment-bias entries are PLLGPU_EUNSUPPORTED. Nothing the context holds is written.
 * The cutting rule. B = the workgroups per (query, candidate), launch_insertions' cut of the site tiles: with
 * T = ceil(sites / 64), 4 x 4: w = ceil(T / 4096), B = ceil(T / (4 w)); every other shape: w = ceil(T / 1024),
 * B = ceil(T / w). QCH = PLLGPU_PLACEMENT_CHUNK_DNA (4 x 4) or PLLGPU_PLACEMENT_CHUNK_TILED queries per workgroup.
 * A launch carries at most PLLGPU_INSERTION_MAX_CANDS descriptors and PLLGPU_INSERTION_MAX_SLOTS partial slots
 * (queries x candidates x B):
 *   C = min(count, MAX_CANDS, max(1, floor(MAX_SLOTS / (B QCH))))                 candidates per launch,
 *   Q = min(queries, QCH min(65535, max(1, floor(floor(MAX_SLOTS / (B C)) / QCH)))) queries per launch,
 * grid (B, C, ceil(Q / QCH)), and the call is ceil(count / C) * ceil(queries / Q) launches (counted into
 * pllgpu_last_launch_count), candidates outermost; one copy back of the whole matrix, one wait. queries == 1 is handed to
 * pllgpu_insertion_loglikelihoods (no node to share; its launches: C = min(count, MAX_CANDS, max(1, floor(MAX_SLOTS / B)))).
 * host_out is written only on success; queries == 0 or count == 0 succeeds without a launch. */
#define PLLGPU_PLACEMENT_CHUNK_DNA 16
#define PLLGPU_PLACEMENT_CHUNK_TILED 4
#define PLLGPU_INSERTION_MAX_CANDS 16384
#define PLLGPU_INSERTION_MAX_SLOTS (4u << 20)
int pllgpu_placement_loglikelihoods(pllgpu_ctx_t *ctx, const unsigned int *query_tips, unsigned int queries,
                                    unsigned int pendant_matrix, const pllgpu_insertion_t *cands, unsigned int count,
                                    const unsigned int *freqs_indices, double *host_out);

/* All three pairings of the four ends around an inner edge, for `count` quartets at once (kernels_quartet.h):
 * host_out[3 i + a] replaces pll_update_partials with two ops into two spare nodes (src/partials.c:237-291) +
 * pll_compute_edge_loglikelihood between them over `inner_matrix` (src/likelihood.c:586-636), for a = 0: ((e0,e1),(e2,e3)),
 * 1: ((e0,e2),(e1,e3)), 2: ((e0,e3),(e1,e2)); the pair that holds e0 is the edge's parent end, the children of a pair stand
 * in the order written. Both nodes exist in registers / LDS only; nothing the context holds is written. is_tip of an end:
 * PLLGPU_QUARTET_TIP_CODES - the end is read as tip codes (its scaler index is not read); PLLGPU_QUARTET_TIP_PATTERN in
 * addition - the reference reads it with its tip kernels (PLL_ATTRIB_PATTERN_TIP), and a pair of two such ends takes no
 * scaling decision, as the reference's tip-tip kernels take none. Every index of the whole list and every tip mark is
 * checked before held work is launched or anything else happens; class-compressed CLVs anywhere in the context and
 * ascertainment-bias entries are PLLGPU_EUNSUPPORTED.
 * The cutting rule. B = the workgroups per quartet, launch_insertions' cut of the site tiles (T = ceil(sites / 64); 4 x 4:
 * w = ceil(T / 4096), B = ceil(T / (4 w)); every other shape: w = ceil(T / 1024), B = ceil(T / w)). A workgroup leaves three
 * partial sums, one per arrangement, and a launch carries at most PLLGPU_QUARTET_MAX descriptors (144 bytes each: one
 * piece of the pinned block) and PLLGPU_INSERTION_MAX_SLOTS partial slots:
 *   Q = min(count, PLLGPU_QUARTET_MAX, max(1, floor(PLLGPU_INSERTION_MAX_SLOTS / (3 B))))   quartets per launch,
 * grid (B, Q), ceil(count / Q) launches (counted into pllgpu_last_launch_count); one copy back of all 3 count values, one
 * wait. Value 3 i + a owns B slots and a ticket of its own: its bits depend on the site count and its own ends alone.
 * host_out is written only on success; count == 0 succeeds without a launch. */
#define PLLGPU_QUARTET_TIP_CODES 1u
#define PLLGPU_QUARTET_TIP_PATTERN 2u
#define PLLGPU_QUARTET_MAX 8192
typedef struct pllgpu_quartet
{
  unsigned int clv[4];
  int scaler[4];
  unsigned int matrix[4];
  unsigned int is_tip[4];
  unsigned int inner_matrix;
} pllgpu_quartet_t;
int pllgpu_quartet_loglikelihoods(pllgpu_ctx_t *ctx, const pllgpu_quartet_t *quartets, unsigned int count,
                                  const unsigned int *freqs_indices, double *host_out);

/* The same launch with every site's value kept, and the sums of those values under `replicates` resampled weight vectors
 * (kernels_quartet.h: the PS instantiations; kernels_resample.h: the contraction). With value v = 3 i + a and u_v[n] the
 * log-likelihood of site n before its pattern weight:
 *   host_lnl[v]                                    what pllgpu_quartet_loglikelihoods gives, bit for bit (same launch geometry, same
 *                                                  hand-off); or NULL
 *   host_persite[v * sites + n]                    u_v[n] * pattern_weights[n], the product formed on the device; or NULL
 *   host_resampled[(i * replicates + b) * 3 + a]   sum_n u_v[n] * weights[b * sites + n] in binary64; required iff replicates > 0
 * weights: [replicates][sites], uploaded as they are and converted on the device; read for n < sites only. All three
 * outputs NULL, or replicates > 0 without weights or host_resampled, is PLLGPU_EINVAL; every other check is
 * pllgpu_quartet_loglikelihoods', in its order. Nothing the context holds is written.
 * Stage 2 splits the sites into S = min(64, ceil(sites / 2048)) ranges of 64 ceil(ceil(sites / S) / 64) sites, a function of
 * the site count alone, and adds the S partials of an element in range order in a second launch: the bits of a resampled
 * value depend on the site count, its own quartet and its own row of weights alone.
 * The cutting rule. M = PLLGPU_RESAMPLE_MAX_BYTES (the environment variable PLL_AMD_RESAMPLE_SCRATCH, read at context
 * creation, lowers it: tests) bounds the scratch of one chunk: per-site rows, weights, partials and results. With
 * P = 64 ceil(sites / 64), W = 4 ceil(sites / 4) and Q0 the quartets per launch of pllgpu_quartet_loglikelihoods:
 *   q = 24 (P if replicates > 0) + 24 (sites if host_persite)         bytes of per-site rows per quartet,
 *   Q = min(count, Q0, max(1, floor(M / 2 / q)))                        quartets per chunk (Q = min(count, Q0) if q = 0),
 *   r = 4 W + 24 Q (S + 1)                                              bytes per replicate: weights, partials, results,
 *   R = min(replicates, max(1, floor((M - q Q) / r)))                   replicates per chunk.
 * Quartets are cut first, then replicates. Replicate chunks are the outer loop, so every row of weights is uploaded once
 * per call; inside, each quartet chunk is one stage-1 launch (skipped from the second replicate chunk on when the
 * quartets are a single chunk: its rows are still there), one contraction and one reduction launch, all counted into
 * pllgpu_last_launch_count, then one copy back of the chunk's per-site rows and one of its sums. 61 quartets x 100 000
 * sites x 1000 replicates is one chunk of each (765 MB with host_persite). The scratch comes from the context's block
 * pool: a second call of the same size allocates nothing.
 * host_lnl and host_resampled are written only on success; host_persite is written chunk by chunk, so after a DEVICE error
 * in a later chunk it may hold the earlier ones (every argument error is found before anything is written).
 * count == 0 succeeds without a launch. */
#define PLLGPU_RESAMPLE_MAX_BYTES ((size_t)1 << 30)
int pllgpu_quartet_resampled_loglikelihoods(pllgpu_ctx_t *ctx, const pllgpu_quartet_t *quartets, unsigned int count,
                                            const unsigned int *freqs_indices, const unsigned int *weights, unsigned int replicates,
                                            double *host_lnl, double *host_resampled, double *host_persite);
/* diagnosis (tools/quartet_resample_probe.py, tools/quartet_rell_probe.py): stream-event times of the last such call's
 * first chunk, in ms - ms[0] what puts the chunk's weights in place (the upload, or the draw of
 * pllgpu_quartet_rell_loglikelihoods), ms[1] the stage-1 launch with its descriptors, ms[2] contraction + reduction */
int pllgpu_resample_last_times(const pllgpu_ctx_t *ctx, double *ms);

/* Replicate weights drawn on the device (kernels_rell.h; DESIGN.md section 5.11 is the definition, pllamd/rell.py restates
 * it in integer arithmetic and the device equals it bit for bit). With p the pattern weights the context holds
 * (pllgpu_pattern_weights_upload), total = sum p and cdf their prefix sums, row b is `total` draws: draw j takes the 64-bit
 * word x(seed, b, j) of Philox-4x32-10, forms r = floor(x total / 2^64) and increments the first site n with cdf[n] > r.
 * b is the ABSOLUTE replicate number: a row is a function of (seed, b, p) and of nothing else - not the chunking, not the
 * number of rows asked for, not the run - so no handle to weights on the device exists; rows are drawn again instead.
 * The prefix sums (k_rell_cdf: one launch, counted, and one read-back of `total`) are formed again when
 * pllgpu_pattern_weights_upload has run since they were last formed and kept otherwise. They live in a buffer of their own,
 * 8 sites + 16 bytes, OUTSIDE the M of the cutting rule above. total == 0 or total >= 2^32 is PLLGPU_EINVAL (a row's words
 * are 32 bits).
 * k_rell_draw fills the rows of the weight scratch the contraction reads, one launch per replicate chunk (counted), grid
 * (rows, ceil(sites / H)): a workgroup counts the draws that fall into its H sites in LDS and stores its part of the row
 * once; no global atomics, no memset. H = 32768 sites (128 KB of LDS); the environment variable PLL_AMD_RELL_RANGE, read at context
 * creation, lowers it to any multiple of 4 >= 4 (tests).
 *
 * pllgpu_replicate_weights_draw: rows [first, first + replicates) of the definition, copied to host_out
 * [replicates][sites]. No quartets, no CLVs; held work stays held. PLLGPU_EUNSUPPORTED for ascertainment-bias entries and
 * class-compressed CLVs, as the quartet calls (the rows could not be fed to them). The rows go through the weight scratch:
 * R = min(replicates, max(1, floor(M / (4 W)))) rows per chunk, one draw launch and one copy back per chunk.
 * replicates == 0 succeeds without a launch.
 *
 * pllgpu_quartet_rell_loglikelihoods: pllgpu_quartet_resampled_loglikelihoods with rows 0 .. replicates - 1 of the
 * definition in place of uploaded ones - the same loop, the same cutting rule (r already holds the 4 W bytes of a row), the
 * same launches plus one draw launch per replicate chunk: 4 launches uncut, 5 when the prefix sums are formed again. The
 * checks, in this order, before anything is launched or written: those of pllgpu_quartet_resampled_loglikelihoods, with
 * "replicates > 0 without host_resampled" in place of "without weights or results"; then, if replicates > 0, the sum of
 * the pattern weights (above). replicates == 0 is that call with replicates == 0. host_weights_out: NULL, or
 * [replicates][sites], filled with one copy back per replicate chunk - like host_persite it may hold earlier chunks after a
 * device error in a later one. */
int pllgpu_replicate_weights_draw(pllgpu_ctx_t *ctx, unsigned long long seed, unsigned int first, unsigned int replicates,
                                  unsigned int *host_out);
int pllgpu_quartet_rell_loglikelihoods(pllgpu_ctx_t *ctx, const pllgpu_quartet_t *quartets, unsigned int count,
                                       const unsigned int *freqs_indices, unsigned long long seed, unsigned int replicates,
                                       double *host_lnl, double *host_resampled, double *host_persite,
                                       unsigned int *host_weights_out);

/* The first and second derivative of -lnL with respect to the branch length, for `count` branches at once
 * (kernels_gradient.h): host_d[i], host_dd[i] replace pllgpu_update_sumtable + pllgpu_likelihood_derivatives for the
 * branch between parent_clv and child_clv at branch_length - but no table exists: a (site, rate) row is formed in
 * registers from the two ends and the two contraction matrices (pllgpu_aux_matrix_upload) and contracted at once with the
 * branch's own (e, l e, l^2 e), which every workgroup forms in LDS from the eigenvalues and rates the context holds.
 * Nothing the context holds is written. parent_is_tip / child_is_tip: the end is read as tip codes and its scaler index is
 * not read; at most one end of a branch may be (PLLGPU_EINVAL). Scalers are read with per-rate scalers only (per-site
 * counts cancel in L'/L): column k of a site is multiplied by 2^(-256 min(s_k - min_k s_k, 4)), s_k the two ends' counts
 * added, as k_sumtable_excess does to a table. Every index, tip mark and length of the whole list is checked before held
 * work is launched or anything else happens; class-compressed CLVs anywhere in the context and ascertainment-bias entries
 * are PLLGPU_EUNSUPPORTED. Held work is launched and pending CLVs are stored first: a branch may name what a traversal
 * produced.
 * The cutting rule. B = the workgroups per branch, launch_insertions' cut of the site tiles (T = ceil(sites / 64); 4 x 4:
 * w = ceil(T / 4096), B = ceil(T / (4 w)); every other shape: w = ceil(T / 1024), B = ceil(T / w)). A workgroup leaves two
 * partial sums, and a launch carries at most PLLGPU_BRANCH_MAX descriptors (64 bytes each: one piece of the pinned block)
 * and PLLGPU_INSERTION_MAX_SLOTS partial slots:
 *   Q = min(count, PLLGPU_BRANCH_MAX, max(1, floor(PLLGPU_INSERTION_MAX_SLOTS / (2 B))))   branches per launch,
 * grid (B, Q), ceil(count / Q) launches (counted into pllgpu_last_launch_count); one copy back of all 2 count values, one
 * wait. Each value owns B slots and a ticket of its own: its bits depend on the site count and its own branch alone.
 * host_d / host_dd (which may be NULL) are written only on success; count == 0 succeeds without a launch. */
#define PLLGPU_BRANCH_MAX 8192
typedef struct pllgpu_branch
{
  unsigned int parent_clv;
  int parent_scaler;
  unsigned int child_clv;
  int child_scaler;
  unsigned int parent_is_tip, child_is_tip;
  double branch_length;
} pllgpu_branch_t;
int pllgpu_branch_derivatives(pllgpu_ctx_t *ctx, const pllgpu_branch_t *branches, unsigned int count,
                              const unsigned int *params_indices, double *host_d, double *host_dd);

/* The same launch keeping what it otherwise drops (kernels_gradient.h, CAT): per branch i and rate category k,
 *   host_d_cat[i][k] = sum_n pw[n] * ( - w_k c1_k[n] / L[n] ),   c1_k after the excess factor and the (1 - pinv) step,
 * category k's share of host_d[i] (sum_k host_d_cat[i][k] = host_d[i] up to rounding), and their contraction with the
 * lengths t_i and the category rates r_k the context holds, formed on the device by k_rate_gradient in list order:
 *   host_d_rates[k] = sum_i (t_i / r_k) * host_d_cat[i][k]      host_d_scale = sum_i t_i * host_d[i]
 * (each product rounded, then added: i = 0 .. count-1). The rates are not checked: a rate of zero gives what the
 * division gives. Any output may be NULL, not all five (PLLGPU_EINVAL, the first check); every other check, the
 * refusals, the flush of held work and the ends are pllgpu_branch_derivatives', through the same code. host_d / host_dd
 * have the bits pllgpu_branch_derivatives gives them, and every host_d_cat value the same bits alone, among others and in
 * any list order.
 * The cutting rule. B as above; with R = rate_cats a workgroup leaves R + 2 partial sums (d_f, dd_f, d_cat[0..R)), each
 * with B slots and a ticket of its own, published at most 32 at a time:
 *   Q = min(count, PLLGPU_BRANCH_MAX, max(1, floor(PLLGPU_INSERTION_MAX_SLOTS / ((R + 2) B))))   branches per launch,
 * grid (B, Q), ceil(count / Q) launches, plus ONE launch of k_rate_gradient (one workgroup, behind the last cut on the
 * same stream, no host wait between; the lengths of all count branches go up once, 8 bytes each) when host_d_rates or
 * host_d_scale is asked for. One copy back of everything, one wait. Every other shape than 4 x 4 keeps 1 KB of LDS per
 * rate category beside the branch's diag table: PLLGPU_EUNSUPPORTED where 32 R (states + 32) bytes exceed 152 KB (the last
 * check: held work has been launched by then, nothing else has happened).
 * count == 0 succeeds without a launch: host_d_rates[0..R) and host_d_scale are set to 0, nothing else is written. */
int pllgpu_branch_category_derivatives(pllgpu_ctx_t *ctx, const pllgpu_branch_t *branches, unsigned int count,
                                       const unsigned int *params_indices, double *host_d_cat, double *host_d, double *host_dd,
                                       double *host_d_rates, double *host_d_scale);

/* The model gradient (kernels_qgradient.h): the derivative of -lnL with respect to every entry of every rate matrix,
 * host_d_q [rate_matrices][states][states], and - host_d_root [rate_matrices][states], or NULL - the explicit dependence of
 * -lnL on the frequencies through the root sum taken at branches[0]; include/pll_amd.h (pll_gpu_qmatrix_gradient) holds the
 * definitions. The list, its checks and their order, the refusals, the flush of held work, what the ends may be and how
 * scalers are read are pllgpu_branch_derivatives', through the same code; host_d_q must not be NULL (PLLGPU_EINVAL). A rate
 * matrix that no category uses gets zeros. The eigenvectors are those of the two contraction matrices
 * (pllgpu_aux_matrix_upload) and the frequencies the context holds. Nothing the context holds is written.
 * The cutting rule. B = the workgroups per branch, a function of the shape alone (T = ceil(sites / 64); 4 x 4: w =
 * ceil(T / (4 PLLGPU_QGRADIENT_MAX_BLOCKS)), B = ceil(T / (4 w)); every other shape: P = states rounded up to a multiple of
 * 16, M = min(PLLGPU_QGRADIENT_MAX_BLOCKS, max(4, floor(16384 / P^2))), w = ceil(T / M), B = ceil(T / w) - 4 workgroups at
 * 61 states). A workgroup leaves V = U states^2 values in a slot of its own, U the number of rate matrices that a category
 * uses, and twice that when host_d_root is asked; a launch carries at most PLLGPU_BRANCH_MAX descriptors and
 * PLLGPU_INSERTION_MAX_SLOTS partial slots:
 *   Q = min(count, PLLGPU_BRANCH_MAX, max(1, floor(PLLGPU_INSERTION_MAX_SLOTS / (V B))))   branches per launch,
 * grid (B, Q). Behind every cut two small launches add the slots of each branch in slot order and the branches in list
 * order; behind the last cut one launch transforms the sums with the eigenvectors: 3 ceil(count / Q) + 1 launches (counted
 * into pllgpu_last_launch_count), no host wait between them, one copy back, one wait. No ticket and no atomic: the bits
 * follow from the shape and the list. Every other shape than 4 x 4 parks both eigenbasis vectors of a tile in LDS:
 * PLLGPU_EUNSUPPORTED where PLLGPU_QGRADIENT_LDS_BYTES = 8 (4 R states + 256 + 64 R + 130 R P) exceed
 * PLLGPU_QGRADIENT_LDS_MAX = 160 KB (the last check here: held work has been launched by then, nothing else has happened;
 * the host layer asks the same question before it asks for the device).
 * count == 0 succeeds without a launch: host_d_q and host_d_root are set to 0. */
#define PLLGPU_QGRADIENT_MAX_BLOCKS 64
#define PLLGPU_QGRADIENT_LDS_MAX (160ul * 1024ul)
#define PLLGPU_QGRADIENT_LDS_BYTES(S, R) (8ul * (4ul * (R) * (S) + 256ul + 64ul * (R) + 130ul * (R) * (((S) + 15ul) / 16ul * 16ul)))
int pllgpu_qmatrix_gradient(pllgpu_ctx_t *ctx, const pllgpu_branch_t *branches, unsigned int count,
                            const unsigned int *params_indices, double *host_d_q, double *host_d_root);

/* replaces pll_compute_node_ancestral[_extbuf] (src/likelihood.c:639-823): the marginal state probabilities of
 * the node at edge->parent_clv, [sites][states] unpadded, given the other end edge->child_clv (a CLV, or tip codes
 * with child_is_tip) across edge->matrix. Of `edge`, gather must be 0 and want_persite / device_result / sequence
 * are not used. Exactly one of the outputs is non-NULL: host_out - the table is copied back and the call waits;
 * device_out - sites * states doubles of DEVICE memory, the call returns once the kernel is enqueued on the
 * context's stream. One launch, counted into pllgpu_last_launch_count. With per-rate scalers the counts of both
 * ends are honoured (kernels_ancestral.h), which the reference does not do.
 * The cutting rule is stage A's of pllgpu_edge_category_posteriors below: 4 x 4 with T = ceil(sites / 64), w =
 * ceil(T / 16384) tiles per wave, ceil(T / (4 w)) workgroups of 256; every other shape w = ceil(T / 4096) tiles per
 * workgroup, ceil(T / w) workgroups of 64 min(rate_cats, 4). */
int pllgpu_node_ancestral(pllgpu_ctx_t *ctx, const pllgpu_edge_t *edge, double *host_out, void *device_out);

/* The per-category site likelihoods of an edge and what model optimisation makes of them (kernels_category.h). With
 * l[n][k] = sum_j pi_f(k)[j] x_k[n][j] (P_k y_k[n])[j], s[n][k] the scaling counts of both ends added (per site, or per
 * rate), c[n] = min_k s[n][k], u = l * 2^(-256 min(s - c, 4)), A[n][k] = w_k (1 - p_f(k)) u[n][k], I[n][k] =
 * w_k p_f(k) pi_f(k)[inv_n] (p_f(k) > 0 and site n invariant, else 0), A multiplied by 2^(-256 min(c, 4)) where c > 0 and
 * sum_k I > 0 (finish_site's rule), L[n] = sum_k (A + I):
 *   cat_lnl[n][k]   = log(l[n][k]) - 256 ln2 * s[n][k]        posterior[n][k] = (A[n][k] + I[n][k]) / L[n]
 *   site_rates[n]   = sum_k (A[n][k] / L[n]) * r_k             weight_sums[k]  = sum_n pw[n] * posterior[n][k]
 *   lnl             = sum_n pw[n] * finish_site(sum_k A, sum_k I, c[n])     (what pllgpu_edge_loglikelihood returns)
 * Host layouts are site-major; each output may be NULL, not all five. A site with L = 0 has a zero row and rate.
 * Of `edge`, gather must be 0 and want_persite / device_result / sequence are not used. Checks, in this order and all
 * before anything is launched: null arguments, the edge's indices (check_edge), class-compressed CLVs and
 * ascertainment-bias entries (PLLGPU_EUNSUPPORTED). Held work is launched and pending CLVs are stored first.
 * The launch rule (counted into pllgpu_last_launch_count). Stage A, one launch, writes the table u as [k][sites rounded
 * up to 64], a count word per site and cat_lnl: 4 x 4 with T = ceil(sites / 64), w = ceil(T / 16384), ceil(T / (4 w))
 * workgroups of 256; every other shape w = ceil(T / 4096), ceil(T / w) workgroups of 64 min(rate_cats, 4). Stage B,
 * k_category_mix, B = min(ceil(sites / 256), 1024) workgroups of 256 walking the 256-site tiles with stride B, mixes
 * the table under one row of weights in device memory and leaves rate_cats + 1 partial sums per workgroup; stage C,
 * k_category_reduce, one workgroup, adds each value's B partials in ascending order. 1 launch when only cat_lnl is asked,
 * 2 with posterior or site_rates, 3 with weight_sums or lnl; then one copy back per output and one wait. Scratch from
 * the context's block pool: 8 rate_cats sites_padded + 4 sites bytes, 8 (rate_cats + 1) B of partials, the staging of
 * the outputs asked for. Outputs are written only on success. */
int pllgpu_edge_category_posteriors(pllgpu_ctx_t *ctx, const pllgpu_edge_t *edge, double *host_cat_lnl, double *host_posterior,
                                    double *host_site_rates, double *host_weight_sums, double *host_lnl);

/* EM on the category weights over the same table: stage A once, then stages B and C `steps + 1` times, evaluation i
 * under row i of a device array [steps + 1][rate_cats] whose row 0 is start_weights and whose row i + 1 stage C forms
 * as S_k / (S_0 + ... + S_{R-1}) (added in that order), S = weight_sums under row i. 1 + 2 (steps + 1) launches with no
 * host wait between them, one copy back of the rows (host_weights, [steps + 1][rate_cats]) and one of the evaluations'
 * lnl (host_lnl, [steps + 1], may be NULL), one wait. The context's rate_weights are neither read nor written. NULL
 * start_weights or host_weights, steps > PLLGPU_EM_MAX_STEPS, a start weight that is negative or not finite or a start
 * row summing to 0 are PLLGPU_EINVAL, before the checks above. */
#define PLLGPU_EM_MAX_STEPS 1024
int pllgpu_category_weights_em(pllgpu_ctx_t *ctx, const pllgpu_edge_t *edge, const double *start_weights, unsigned int steps,
                               double *host_weights, double *host_lnl);

/* ---- transition matrices on the device ---------------------------- */
/* eigensystem of rate matrix `index` in the reference's layouts: eigenvecs[j*sp+i],
 * inv_eigenvecs[i*sp+j] ([states][states_padded] each), eigenvals[states_padded] */
int pllgpu_eigen_upload(pllgpu_ctx_t *ctx, unsigned int index, const double *eigenvecs,
                        const double *inv_eigenvecs, const double *eigenvals);
/* replaces pll_core_update_pmatrix (src/core_pmatrix.c:24-258): P = I + Vinv' diag(expm1(lambda r t /
 * (1 - pinv))) V per (matrix, rate category), identity for t = 0, written straight into the
 * device's transposed layout. Needs the eigensystems, category rates (pllgpu_rates_upload) and
 * prop_invar on the device. Asynchronous. */
int pllgpu_update_pmatrices(pllgpu_ctx_t *ctx, const unsigned int *params_indices /* [rate_cats] */,
                            const unsigned int *matrix_indices, const double *branch_lengths,
                            unsigned int count);
/* device matrix `index` back in the reference's host layout [rate][row][states_padded]. Synchronises. */
int pllgpu_pmatrix_download(pllgpu_ctx_t *ctx, unsigned int index, double *host);

/* ascertainment-bias correction (src/likelihood.c:50-120, :191-268,
 * :342-440): for each state n the likelihood of the per-state extra entry `sites + n` of the same
 * edge (is_root = 0; edge->child_is_tip honoured) or root (is_root = 1; only parent_clv /
 * parent_scaler / freqs_indices of `edge` are read) and the number of scalings it carries.
 * With per-rate scalers the term is already brought to the smallest per-rate count, which is the
 * count reported. Synchronises. */
int pllgpu_asc_terms(pllgpu_ctx_t *ctx, const pllgpu_edge_t *edge, int is_root, double *terms /* [states] */,
                     unsigned int *scalings /* [states] */);

/* ---- branch-length derivatives ---------------------------------- */
/* the two contraction matrices of the sumtable, one block [rate][row j][states_padded] each:
 * slot 0: M1[j][i] = pi_i * inv_eigenvecs[i][j] (applied to the left end), slot 1: M2[j][i] =
 * eigenvecs[j][i] (right end) - src/core_derivatives.c:446-456 */
int pllgpu_aux_matrix_upload(pllgpu_ctx_t *ctx, unsigned int slot, const double *host_block);
int pllgpu_eigenvals_upload(pllgpu_ctx_t *ctx, unsigned int index, const double *host);
int pllgpu_rates_upload(pllgpu_ctx_t *ctx, const double *host); /* category rates [rate_cats] */
typedef struct pllgpu_sumtable
{
  unsigned int left_clv, right_clv; /* a tip given by codes must be the left end */
  int left_scaler, right_scaler;
  unsigned int left_is_tip;
  unsigned int gather;
} pllgpu_sumtable_t;
/* replaces pll_core_update_sumtable_{ii,ti,repeats} (src/core_derivatives.c:25-641); the table
 * stays in HBM in one of PLLGPU_SUMTABLE_SLOTS slots (allocated on first use) */
#define PLLGPU_SUMTABLE_SLOTS 16
int pllgpu_update_sumtable(pllgpu_ctx_t *ctx, const pllgpu_sumtable_t *st, unsigned int slot);
int pllgpu_sumtable_upload(pllgpu_ctx_t *ctx, unsigned int slot, const double *host);
int pllgpu_sumtable_download(pllgpu_ctx_t *ctx, unsigned int slot, double *host);
/* give the slot's HBM back (pll_gpu_release_sumtable) */
int pllgpu_sumtable_release(pllgpu_ctx_t *ctx, unsigned int slot);
/* replaces pll_core_likelihood_derivatives (src/core_derivatives.c:696-849). Synchronises. */
/* eval_sites: how many leading table entries enter the sums (sites, or sites + states for the
 * Stamatakis correction, src/core_derivatives.c:733-742) */
int pllgpu_likelihood_derivatives(pllgpu_ctx_t *ctx, unsigned int slot, double branch_length,
                                  const unsigned int *params_indices, unsigned int eval_sites, double *d_f,
                                  double *dd_f);
/* Safeguarded Newton iteration for the branch length of the slot's table, run on the device: one launch per
 * evaluation chained on the context's stream (two where rate_cats * states > 1024: the diag table has its own), the
 * step taken by the workgroup that finishes the sums, no host wait between the launches of a batch of 8; behind each
 * batch a publish step and one poll of mapped memory (host_waits counts them). With matrix_index >= 0 the transition
 * matrix of result.t is left in that slot by a k_pmatrix launch that reads t from the device (not waited for). The
 * recipe, the statuses and the meaning of the fields: pll_gpu_optimize_branch_length (pll_amd.h), whose structs these
 * mirror. Options out of range: PLLGPU_EINVAL before anything is launched. *result and trace (NULL, or 3 * max_iters
 * doubles) are written only on success. Launches counted into pllgpu_last_launch_count. */
#define PLLGPU_NEWTON_MAX_ITERS 64
#define PLLGPU_NEWTON_CONVERGED 0
#define PLLGPU_NEWTON_AT_MIN 1
#define PLLGPU_NEWTON_AT_MAX 2
#define PLLGPU_NEWTON_STALLED 3
#define PLLGPU_NEWTON_MAXITER 4
typedef struct pllgpu_newton
{
  double t_start, t_min, t_max, tolerance;
  unsigned int max_iters;
  int matrix_index;
} pllgpu_newton_t;
typedef struct pllgpu_newton_result
{
  double t, d_f, dd_f;
  unsigned int iterations, host_waits;
  int status;
} pllgpu_newton_result_t;
int pllgpu_optimize_branch_length(pllgpu_ctx_t *ctx, unsigned int slot, const unsigned int *params_indices,
                                  unsigned int eval_sites, const pllgpu_newton_t *options, pllgpu_newton_result_t *result,
                                  double *trace);

/* Maximum-likelihood distances between the tips of a list (kernels_distance.h; include/pll_amd.h, pll_gpu_pairwise_distances,
 * holds the definitions): for list positions x < y the branch length at which the recipe of pllgpu_optimize_branch_length
 * stops on the tip-tip function of (tips[x], tips[y]), tips[x] in the left role (contraction matrix 0 of
 * pllgpu_aux_matrix_upload), with the options of `options` for every pair; matrix_index must be -1. Every tip must have
 * codes on the device (pllgpu_tipchars_upload) and, for other than 4 states, the code -> mask map must be there
 * (pllgpu_tipmap_upload). The outputs are [count][count] host arrays, [x][y] and [y][x] written from one computation, the
 * diagonal 0; all but distance may be NULL. Nothing the context holds is written.
 * Two things the context cannot see are the caller's to hold: prop_invar of every used rate matrix is 0 (the invariant term
 * belongs to the alignment column, not to the code pair) and the pattern weights add up to less than 2^32 (the counts are
 * 32-bit words). The host layer refuses both.
 * The checks, before held work is launched or anything else happens, in this order: PLLGPU_EINVAL for a NULL out or
 * distance, with count > 0 a NULL tips, params_indices or options, a tips[i] >= tips, options out of range (those of
 * pllgpu_optimize_branch_length, and matrix_index != -1), a params_indices[k] out of range, a tip without codes on the
 * device; PLLGPU_EUNSUPPORTED for ascertainment-bias entries, class-compressed CLVs anywhere in the context, and a code
 * table beyond the limit. The limit. C = the codes in use (16 for 4 states, else 1 + the highest code with a non-empty
 * mask). A workgroup keeps the diag table of its pair and at least one table of C^2 counts in LDS:
 *   C <= PLLGPU_DISTANCE_MAX_CODES   and   PLLGPU_DISTANCE_LDS_BYTES = 32 R states + 4 (C^2 | 1) <= PLLGPU_DISTANCE_LDS_MAX.
 * (61 states x 4 categories with 64 codes: 24 KB.) Where there is room a workgroup keeps 2, 4, ... 256 such tables, up to 36 KB
 * of them, one per thread modulo their number: counts are integers, so their number changes no bit.
 * The cutting rule. One workgroup per pair, grid (count, rows): workgroup (y, x - row0) serves the pair x < y and every
 * other one returns at once. A launch carries whole rows of the pair matrix,
 *   rows = max(1, min(65535, floor(PLLGPU_DISTANCE_MAX_PAIRS / count)))   rows per launch,
 * ceil((count - 1) / rows) launches behind ONE launch of k_distance_code_vectors: 1 + ceil((count - 1) / rows) in all
 * (counted into pllgpu_last_launch_count), no host wait between them, one copy back of all 6 count^2 values, one wait. A
 * pair's bits depend on its two code rows, the model and the options alone.
 * count == 0 succeeds at once, nothing but out and distance looked at; count == 1 succeeds without a launch once the
 * arguments themselves have passed (the checks up to params_indices), the one diagonal entry of every output set to 0.
 * PLL_AMD_DISTANCE_PAIRS in the environment of the context's creation lowers PLLGPU_DISTANCE_MAX_PAIRS in the rule above
 * (tests: a small list over several launches). */
#define PLLGPU_DISTANCE_MAX_CODES 128
#define PLLGPU_DISTANCE_LDS_MAX (158ul * 1024ul)
#define PLLGPU_DISTANCE_LDS_BYTES(S, R, C) (32ul * (R) * (S) + 4ul * (((C) * (C)) | 1ul))
#define PLLGPU_DISTANCE_MAX_PAIRS (1u << 20)
typedef struct pllgpu_distances
{
  double *distance, *p_distance, *d_f, *dd_f;
  int *status;
  unsigned int *iterations;
} pllgpu_distances_t;
int pllgpu_pairwise_distances(pllgpu_ctx_t *ctx, const unsigned int *tips, unsigned int count, const unsigned int *params_indices,
                              const pllgpu_newton_t *options, const pllgpu_distances_t *out);

/* Neighbour-joining (flags 0) and BIONJ (PLLGPU_NJ_BIONJ) trees from distances (kernels_nj.h; include/pll_amd.h,
 * pll_gpu_nj_tree, holds the tree format and pllamd/nj.py the definition, operation for operation).
 * pllgpu_nj_tree needs no context: it owns a stream and its blocks on `device` (-1: PLL_AMD_DEVICE, else the calling
 * thread's current device) for the length of the call, copies host_dist ([count][count]; only [x][y], x < y, is read) up and
 * parent / length ([2 count - 2] each) back, and leaves the thread's device as it found it. pllgpu_distance_tree is
 * pllgpu_pairwise_distances' checks and launches followed by the same join on the distance block where it lies (the first
 * count^2 doubles of the call's results); the join's working set comes from the context's block pool and returns to it,
 * nothing the context holds is written, and host_dist_or_NULL receives the [count][count] distances. Both are one routine on
 * (device matrix, stream, block). Synchronous: one wait at the end; outputs are written only on success.
 * Working set: 8 count^2 bytes (twice that for BIONJ) + O(count).
 * The launch rule. count == 3: ONE launch (the three-node step). count >= 4: one launch that copies the upper triangle into
 * both halves of the working matrix and forms the first row sums, per join one search launch (ceil((r - 1) / rows)
 * workgroups at r active nodes, rows = PLLGPU_NJ_ROWS, the last to take the step's ticket leaves the step's record) and one
 * join launch (ceil(r / 256) workgroups), then the three-node step:
 *   2 (count - 3) + 2   launches,
 * no host wait between them. pllgpu_nj_last_launch_count reports them for the calling thread's last pllgpu_nj_tree (0 after a
 * failure); pllgpu_distance_tree counts them into pllgpu_last_launch_count behind those of the distances.
 * PLL_AMD_NJ_ROWS in the environment, read when a call starts, lowers PLLGPU_NJ_ROWS (tests: nine nodes over several search
 * workgroups and the ticket); the answer's bits do not depend on it.
 * The checks, before anything is launched: PLLGPU_EINVAL for a NULL host_dist, parent or length, count < 3, unknown flag
 * bits, a device out of range; PLLGPU_ENODEVICE without a device. pllgpu_distance_tree: NULL parent or length, then the
 * argument checks of pllgpu_pairwise_distances, then count < 3 and the flags, then the remaining checks of
 * pllgpu_pairwise_distances. The entries' values are the host layer's to check (finite, not negative); a step whose
 * criterion holds no number fails the call with PLLGPU_ERUNTIME instead of joining anything. */
#define PLLGPU_NJ_BIONJ 1u
#define PLLGPU_NJ_ROWS 8u
int pllgpu_nj_tree(int device, const double *host_dist, unsigned int count, unsigned int flags, int *parent, double *length);
int pllgpu_distance_tree(pllgpu_ctx_t *ctx, const unsigned int *tips, unsigned int count, const unsigned int *params_indices,
                         const pllgpu_newton_t *options, unsigned int flags, int *parent, double *length, double *host_dist_or_NULL);
unsigned int pllgpu_nj_last_launch_count(void);
/* milliseconds from the first to the last launch of the calling thread's last join (either entry point), by device events
 * on the call's stream; -1 when no join ran or the events could not be had (tools/nj_probe.py) */
double pllgpu_nj_last_device_ms(void);

/* Many trees in one call (include/pll_amd.h, pll_gpu_nj_trees and pll_gpu_bootstrap_distance_trees,
 * hold the contracts). All matrices of a call have the same count, so step s of every join has the same r: the four
 * kernels take the replicate from the second grid dimension, replicate b's working set (matrices, row sums, labels,
 * tickets, partials, step record, parent, length, status word) lying pllgpu_nj_scratch_bytes(count, flags) bytes times b
 * behind the first. Tree b has bit for bit what pllgpu_nj_tree gives on matrix b; pllgpu_nj_tree IS this routine with one
 * replicate.
 * pllgpu_nj_trees: host_dist [replicates][count][count], parent / length [replicates][2 count - 2]; the checks and the
 * device are pllgpu_nj_tree's, replicates == 0 succeeds behind the argument checks with nothing written. The replicates
 * are cut into chunks of
 *   n = min(replicates, 65535, max(1, floor(PLLGPU_NJ_BATCH_MAX_BYTES / (8 count^2 + pllgpu_nj_scratch_bytes))))
 * matrices; a chunk is one copy up, one memset of all tickets and status words, the launch sequence of pllgpu_nj_tree with
 * grids (x, n), one copy back each of parents, lengths and status words, one wait:
 *   chunks x (2 (count - 3) + 2)   launches   (chunks x 1 at count == 3),
 * whatever n is; pllgpu_nj_last_launch_count reports them. PLL_AMD_NJ_BATCH_BYTES in the environment, read when a call
 * starts, lowers the budget (tests). A replicate whose search finds no pair fails the call with PLLGPU_ERUNTIME, the
 * message naming the first such replicate; outputs are written only when every chunk has succeeded.
 *
 * pllgpu_bootstrap_distance_trees: for b < replicates, row first + b of pllgpu_replicate_weights_draw(seed) in the place
 * of the pattern weights, pllgpu_pairwise_distances' launches under that row (k_pairwise_distances_rows: the one body of
 * k_pairwise_distances over (weight row, result block), the replicate the grid's third dimension), and the join of the
 * replicate's distance plane where it lies. Nothing the context holds is written, the pattern weights included; the rows
 * never leave the device unless out->weights asks for them. With W = sites rounded up to 4 the replicates are cut into
 * chunks of
 *   n = min(replicates, 65535, max(1, floor(PLLGPU_BOOTSTRAP_MAX_BYTES / (4 W + 48 count^2 + pllgpu_nj_scratch_bytes))))
 * whose blocks come from the context's block pool and return to it. PLL_AMD_BOOTSTRAP_BYTES in the environment of the
 * context's creation lowers the budget (tests).
 * The launch rule. Once per call: k_rell_cdf if the pattern weights were uploaded since the prefix sums were last formed
 * (0 or 1), and ONE launch of k_distance_code_vectors. Per chunk, on the context's stream with no host wait inside: one
 * k_rell_draw launch; the pair launches, each of at most P = PLLGPU_DISTANCE_MAX_PAIRS workgroups counted as cells x
 * replicates and cut over replicates first, then over rows -
 *   rows = max(1, min(65535, floor(P / count)));
 *   rows >= count - 1 (a matrix fits a launch): ceil(n / m) launches of grid (count, count - 1, <= m),
 *                                               m = max(1, min(65535, floor(P / (count (count - 1)))));
 *   else: n x ceil((count - 1) / rows) launches of grid (count, <= rows, 1);
 * then the 2 (count - 3) + 2 launches of the join (1 at count == 3); then the copies back that were asked for and one wait.
 * Within a chunk the count depends on n through the cap P alone. pllgpu_last_launch_count reports the sum.
 * The checks, before held work is launched: PLLGPU_EINVAL for a NULL out, parent or length; replicates == 0 succeeds here;
 * then those of pllgpu_distance_tree in its order; then the sum of the pattern weights as pllgpu_replicate_weights_draw
 * checks it (which may form the prefix sums: the host layer refuses a sum of 0 before that). Outputs of a chunk are written
 * once the chunk has succeeded: after a device error in a later chunk the rows of earlier ones stay written.
 * pllgpu_bootstrap_last_times: stream-event times of the last such call's first chunk, in ms - ms[0] the draw, ms[1] the
 * pair launches, ms[2] the join (tools/bootstrap_trees_timing.py). */
#define PLLGPU_NJ_BATCH_MAX_BYTES ((size_t)1 << 30)
#define PLLGPU_BOOTSTRAP_MAX_BYTES ((size_t)1 << 30)
typedef struct pllgpu_bootstrap_trees
{
  int *parent;
  double *length;
  double *distances;     /* NULL or [replicates][count][count] */
  int *status;           /* NULL or [replicates][count][count] */
  unsigned int *weights; /* NULL or [replicates][sites] */
} pllgpu_bootstrap_trees_t;
size_t pllgpu_nj_scratch_bytes(unsigned int count, unsigned int flags);
int pllgpu_nj_trees(int device, const double *host_dist, unsigned int count, unsigned int replicates, unsigned int flags, int *parent,
                    double *length);
int pllgpu_bootstrap_distance_trees(pllgpu_ctx_t *ctx, const unsigned int *tips, unsigned int count, const unsigned int *params_indices,
                                    const pllgpu_newton_t *options, unsigned int flags, unsigned long long seed, unsigned int first,
                                    unsigned int replicates, const pllgpu_bootstrap_trees_t *out);
int pllgpu_bootstrap_last_times(const pllgpu_ctx_t *ctx, double *ms);

/* (L, L', L'') of the per-state extra entries at the branch length of the LAST
 * pllgpu_likelihood_derivatives call on this context, and their scaling counts
 * (src/core_derivatives.c:864-891). Synchronises. */
int pllgpu_asc_derivative_terms(pllgpu_ctx_t *ctx, unsigned int slot, int parent_scaler, int child_scaler,
                                const unsigned int *params_indices, double *lk /* [states][3] */,
                                unsigned int *scalings /* [states] */);

/* ---- site-pattern compression (src/compress.c:171-410) ------------- */
/* encoded: [count][length] bytes, one row per sequence (characters already recoded). Outputs:
 * compressed [count][*patterns_out] (row stride = *patterns_out) = the unique columns in
 * lexicographic order of the characters taken as signed char, weights[*patterns_out] their
 * multiplicities, site_pattern_map[length] (or NULL) the pattern of every original site. No
 * context: the call owns a stream on `device` (-1: PLL_AMD_DEVICE or 0). Synchronous. */
int pllgpu_compress_patterns(const unsigned char *encoded, unsigned int count, unsigned int length,
                             unsigned char *compressed, unsigned int *weights,
                             unsigned int *site_pattern_map, unsigned int *patterns_out, int device);
const char *pllgpu_compress_last_error(void);

/* ---- the flat seam's tip-tip pair (src/pll.h:1049-1071, src/core_partials.c:1013-1210, :82-200) --------------
 * The caller's lookup table in the REFERENCE's layout: entry (j, k) of two tip codes at index (j << ceil(log2(ncodes)))
 * + k (16 j + k for 4 states, where the code is the state mask) of rate_cats x states_padded doubles = the parent entry
 * of a cherry showing j and k. Matrices in the caller's layout [rate][row][states_padded]. Both calls synchronise. */
int pllgpu_create_lookup(pllgpu_ctx_t *ctx, double *lookup_host, const double *left_host, const double *right_host,
                         const unsigned long long *tipmap_host, unsigned int ncodes);
int pllgpu_tt_from_lookup(pllgpu_ctx_t *ctx, double *parent_host, const unsigned char *left_codes,
                          const unsigned char *right_codes, const double *lookup_host, unsigned int sites, unsigned int ncodes);

/* ---- fast parsimony (src/fast_parsimony.c; csrc/hip/kernels_parsimony.h) ----------------------------------------
 * A record of its own, independent of any pllgpu_ctx (the reference's pll_parsimony_t outlives the partition it was
 * made from): a device, a stream and one block holding the packed vectors of `nodes` nodes - `states` rows of `words`
 * 32-bit words each, state-major as in the reference - and their costs. Vectors and costs start as zero. Node indices
 * are checked against `nodes` before anything is launched. */
typedef struct pllgpu_pars pllgpu_pars_t;
pllgpu_pars_t *pllgpu_pars_create(int device, unsigned int states, unsigned int words, unsigned int nodes);
void pllgpu_pars_destroy(pllgpu_pars_t *pars);
/* host[n] = the vector of node n in the reference's layout ([states][words], src/fast_parsimony.c:286-360), for
 * n in [first, first + count): one copy for all of them. Both synchronise. download also fills cost_host[n]. */
int pllgpu_pars_upload(pllgpu_pars_t *pars, unsigned int first, unsigned int count, unsigned int *const *host);
int pllgpu_pars_download(pllgpu_pars_t *pars, unsigned int first, unsigned int count, unsigned int *const *host,
                         unsigned int *cost_host);
/* replaces pll_fastparsimony_update_vector[_4x4] (src/fast_parsimony.c:458-521, :557-609) for a whole list: ops sorted
 * by level, the ops of one level mutually independent (an op may name its parent as one of its children). One memset
 * and one launch per level; asynchronous on the record's stream. */
typedef struct pllgpu_pars_op
{
  unsigned int parent, child1, child2;
  unsigned int level;
} pllgpu_pars_op_t;
int pllgpu_pars_update(pllgpu_pars_t *pars, const pllgpu_pars_op_t *ops, unsigned int count);
/* replaces pll_fastparsimony_edge_score[_4x4] (src/fast_parsimony.c:405-456, :611-648) for `count` pairs
 * (pairs[2i], pairs[2i+1]): mismatches + both costs + const_cost. One launch, one copy back; synchronises. */
int pllgpu_pars_edge_scores(pllgpu_pars_t *pars, const unsigned int *pairs, unsigned int count, unsigned int const_cost,
                            unsigned int *scores_host);
/* replaces the update_vector + edge_score pair of a stepwise-addition step (src/stepwise.c:507-512) for `count`
 * candidate edges (edges[2i], edges[2i+1]) and one node; the parent vector of each edge stays in registers. One
 * launch, one copy back; synchronises. */
int pllgpu_pars_insertion_scores(pllgpu_pars_t *pars, unsigned int node, const unsigned int *edges, unsigned int count,
                                 unsigned int const_cost, unsigned int *scores_host);
/* what pll_fastparsimony_root_score reads (src/fast_parsimony.c:776-781): four bytes back, no launch; synchronises */
int pllgpu_pars_node_cost(pllgpu_pars_t *pars, unsigned int node, unsigned int *cost_host);
int pllgpu_pars_synchronize(pllgpu_pars_t *pars);
/* kernel launches of the last update / scores call on the record */
unsigned int pllgpu_pars_last_launch_count(const pllgpu_pars_t *pars);

/* ---- weighted (Sankoff) parsimony (src/parsimony.c:117-383; csrc/hip/kernels_sankoff.h) -------------------------
 * The record behind a structure made by pll_parsimony_create: a device (device < 0: PLL_AMD_DEVICE or the calling
 * thread's current one, as pllgpu_create picks it), a stream, `buffers` score buffers, `ancestral_buffers` ancestral
 * buffers and the states x states cost matrix. Score buffers live in the tiled sites-contiguous layout of the CLVs - a
 * tile of 64 sites as [state][64 lanes] doubles - and start as zero, like the ancestral buffers. states 1..64. Score
 * indices are checked against `buffers`, ancestral indices (counted from the first ancestral buffer) against
 * `ancestral_buffers`, before anything is launched. */
typedef struct pllgpu_spars pllgpu_spars_t;
pllgpu_spars_t *pllgpu_spars_create(int device, unsigned int states, unsigned int sites, unsigned int buffers,
                                    unsigned int ancestral_buffers, const double *matrix);
void pllgpu_spars_destroy(pllgpu_spars_t *spars);
/* host[indices[i]] = buffer indices[i] in the reference's layout ([site][state], src/parsimony.c:155-175), i < count:
 * one copy for all of them and one transposing launch (k_sankoff_upload / k_sankoff_download; not counted by
 * pllgpu_spars_last_launch_count). Both synchronise. */
int pllgpu_spars_upload(pllgpu_spars_t *spars, const unsigned int *indices, unsigned int count, double *const *host);
int pllgpu_spars_download(pllgpu_spars_t *spars, const unsigned int *indices, unsigned int count, double *const *host);
/* ancestral buffers [first, first + count) in one copy; host[i] (indexed like the buffers, NULL: skip) receives `sites`
 * words. Synchronises. */
int pllgpu_spars_download_ancestral(pllgpu_spars_t *spars, unsigned int first, unsigned int count, unsigned int *const *host);
/* replaces pll_parsimony_build (src/parsimony.c:204-284) for a list sorted by level, the ops of one level mutually
 * independent (an op may name its parent as one of its children): one launch per level, then the score of
 * score_index (below). Synchronises. */
int pllgpu_spars_build(pllgpu_spars_t *spars, const pllgpu_pars_op_t *ops, unsigned int count, unsigned int score_index,
                       double *score_host);
/* replaces pll_parsimony_score (src/parsimony.c:286-307): one launch, 8 bytes back. min(tiles, 1024) workgroups of one
 * wave walk the site tiles with that stride; their partial sums are added in index order by the one that arrives last,
 * so the bits of the result depend on the site count alone. Synchronises. */
int pllgpu_spars_score(pllgpu_spars_t *spars, unsigned int index, double *score_host);
/* replaces pll_parsimony_reconstruct (src/parsimony.c:309-383) for a list sorted by level: one launch per level.
 * root != 0: the operation reads no parent (the first of a call). tables: 256 words state -> character (the reference's
 * revmap), then 256 words character -> state, each < states. Synchronises. */
typedef struct pllgpu_spars_recop
{
  unsigned int node_score, node_ancestral, parent_score, parent_ancestral;
  unsigned int root;
  unsigned int level;
} pllgpu_spars_recop_t;
int pllgpu_spars_reconstruct(pllgpu_spars_t *spars, const pllgpu_spars_recop_t *ops, unsigned int count, const unsigned int *tables);
/* scores_host[i] = what pll_parsimony_build returns for {{t1, edges[2i], edges[2i+1]}, {t2, t1, node}}; t1 stays in LDS,
 * t2 is never formed, nothing is written but the scores. One launch for up to min(4096, 65536 / w) candidates, w =
 * min(tiles, 64) the workgroups a candidate gets (every candidate owns w partial-sum slots and a ticket; 65536 slots and
 * 4096 tickets exist); a longer list is cut into launches of that many, in list order. A candidate's sum is formed by its
 * own workgroups in slot order: the same bits alone, among others and in any list order. One copy back; synchronises;
 * scores_host is written only on success. */
int pllgpu_spars_insertion_scores(pllgpu_spars_t *spars, unsigned int node, const unsigned int *edges, unsigned int count,
                                  double *scores_host);
int pllgpu_spars_synchronize(pllgpu_spars_t *spars);
/* kernel launches of the last build / score / reconstruct / insertion call on the record */
unsigned int pllgpu_spars_last_launch_count(const pllgpu_spars_t *spars);
/* a call begins: whatever fails before its first launch leaves the count at zero */
void pllgpu_spars_clear_launch_count(pllgpu_spars_t *spars);

/* ---- the exchange of a site-sharded run (pll_gpu_edge_loglikelihood_allreduce) ---------------- */
/* make the context's device the calling thread's current one while a collective library enqueues on the context's
 * stream from the host side of this boundary; *previous (-1: nothing changed) goes to pllgpu_leave_device afterwards */
int pllgpu_enter_device(pllgpu_ctx_t *ctx, int *previous);
void pllgpu_leave_device(int previous);
/* two doubles of device memory owned by the context: {lnL, sequence}, the operand of the all-reduce */
double *pllgpu_reduce_buffer(pllgpu_ctx_t *ctx);
/* after the collective has been enqueued on the context's stream: a one-lane kernel copies the reduced
 * pair to mapped host memory (value first, sequence word behind it) and the call polls for
 * expected_sequence (= ranks x the sequence every rank used). Never synchronises: a collective that a peer does not
 * join never completes, so after 50 ms the poll turns to hipStreamQuery and gives up with PLLGPU_ERUNTIME after
 * timeout_ms (<= 0: 60 s); a drained stream with another sequence word = the ranks are out of step. */
int pllgpu_reduce_fetch(pllgpu_ctx_t *ctx, double expected_sequence, double *value_out, int timeout_ms);
/* a rank whose evaluation failed: {-inf, sequence} as its operand, so that it still takes part in the collective */
int pllgpu_reduce_poison(pllgpu_ctx_t *ctx, double sequence);

/* ---- stream / timing ---------------------------------------------------------------------- */
int pllgpu_set_stream(pllgpu_ctx_t *ctx, void *hip_stream);
void *pllgpu_get_stream(const pllgpu_ctx_t *ctx);
int pllgpu_synchronize(pllgpu_ctx_t *ctx);
int pllgpu_timer_start(pllgpu_ctx_t *ctx);
double pllgpu_timer_stop(pllgpu_ctx_t *ctx); /* ms, < 0 on error */
unsigned int pllgpu_last_launch_count(const pllgpu_ctx_t *ctx);
/* HBM bytes the kernels of the last pllgpu_update_partials call had to move by construction
 * (child reads + parent and scaler writes of every launch as it was grouped) */
double pllgpu_last_algorithmic_bytes(const pllgpu_ctx_t *ctx);
/* CLVs the last whole-traversal launch formed and did not store (stored on demand by whatever may read them) */
unsigned pllgpu_pending_clvs(const pllgpu_ctx_t *ctx);

/* Test hook, host logic only (no device is touched): how pllgpu_update_partials partitions a
 * 4-state x 4-rate op list - classified and level-sorted like the ones the host layer hands over -
 * into chains. Returns the number of launch stages, or 0 when the list does not
 * qualify (anything but producer -> consumer dependencies: it goes through the level scheduler).
 * Per op (arrays of `count`, any may be NULL): stage = the launch it runs in (1-based);
 * chain = its chain's number, -1 for a member of a seven-op group, -2 for an op formed on the fly as
 * another chain's sibling; form = 0 top of a chain, 1 lower step, 2 formed on the fly, 3 group member. */
int pllgpu_debug_chain_plan(const pllgpu_op_t *ops, unsigned int count, unsigned int nodes, unsigned int scale_buffers, int fuse_cc,
                            unsigned int *stage, int *chain, unsigned char *form);

#ifdef __cplusplus
}
#endif
#endif
