// pllgpu.hip - device context, data movement and kernel launches behind include/pll_amd_device.h.
// gfx950 (MI355X) only. No CPU path lives here: every compute entry point launches HIP kernels
// or fails with an error.
#include "../../../include/pll_amd_device.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <thread>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <type_traits>
#include <vector>

#include "kernels_common.h"
#include "kernels_dna.h"
#include "kernels_generic.h"
#include "kernels_deriv.h"
#include "kernels_mfma.h"
#include "kernels_mfma_wide.h"
#include "kernels_lean.h"
#include "kernels_repeats.h"
#include "kernels_ancestral.h"
#include "kernels_category.h"
#include "kernels_parsimony.h"
#include "kernels_sankoff.h"
#include "kernels_insertion.h"
#include "kernels_placement.h"
#include "kernels_quartet.h"
#include "kernels_resample.h"
#include "kernels_rell.h"
#include "kernels_gradient.h"
#include "kernels_qgradient.h"
#include "kernels_distance.h"
#include "kernels_nj.h"

// ---------------------------------------------------------------------------------------------
static thread_local char g_err[256] = "";

static int fail(int code, const char *fmt, ...)
{
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}

#define HIP_TRY(call)                                                                            \
  do                                                                                             \
  {                                                                                              \
    hipError_t e_ = (call);                                                                      \
    if (e_ != hipSuccess)                                                                        \
      return fail(e_ == hipErrorOutOfMemory ? PLLGPU_ENOMEM : PLLGPU_ERUNTIME, "%s failed: %s",   \
                  #call, hipGetErrorString(e_));                                                 \
  } while (0)

// Cached launch plans hold raw device pointers: whenever one of a context's blocks is (re)allocated or freed, THAT
// context's epoch moves (pllgpu_ctx::alloc_epoch) and its plans are planned again. Round 5 kept one counter for the
// whole process, so a partition created, grown or destroyed anywhere - the usual shape of a multi-partition caller, or a
// flat pll_core_* call beside a partition - dropped every other partition's plans. A DevBuf does not know its owner:
// the entry point that is running says whose blocks are being touched (DeviceScope sets t_epoch; a context is used by
// one thread at a time, so the counter is plain).
static unsigned long long g_orphan_epoch = 1; // blocks touched outside any entry point (none today)
static thread_local unsigned long long *t_epoch = &g_orphan_epoch;

// Device blocks a context has let go of are kept for its next request instead of going back to the runtime: hipFree
// waits for the whole device (35 us on average, 0.5 ms at worst, measured under a tree search on a site-repeats partition
// - every move re-orients nodes whose class counts, and so their CLV / map buffers, change size: 9 pairs of hipFree +
// hipMalloc per move, 330 us of a 450 us move; profiles/r6_tree_search.json). Everything a context does is ordered by its
// one stream, so a block may serve its next owner at once: whatever was enqueued to read the old contents runs before
// whatever is enqueued to write the new ones. Sizes are rounded up to four significant bits (at most 1/8 more), so that
// blocks of nearly the same size are interchangeable; what is held idle is bounded (a quarter of what the context's
// buffers hold, and a failed hipMalloc gives everything back and tries again); pllgpu_destroy returns it all.
struct BlockPool
{
  std::multimap<size_t, void *> idle; // bytes -> block
  size_t idle_bytes = 0;
  size_t live_bytes = 0;              // blocks the context's buffers hold
  void trim(size_t keep)
  {
    while (idle_bytes > keep && !idle.empty())
    {
      auto it = std::prev(idle.end()); // the largest first
      (void)hipFree(it->second);
      idle_bytes -= it->first;
      idle.erase(it);
    }
  }
};
// idle blocks a context may hold: a quarter of what its buffers hold (at least 64 MB, at most 8 GB) - many partitions of a
// multi-partition caller must not each sit on gigabytes they once needed
constexpr size_t kPoolIdleMax = (size_t)8 << 30, kPoolIdleMin = (size_t)64 << 20;
static thread_local BlockPool *t_pool = nullptr; // the running entry point's context (DeviceScope), like t_epoch

static inline size_t block_bytes(size_t bytes)
{
  if (bytes <= 4096) return 4096;
  int top = 63 - __builtin_clzll((unsigned long long)bytes);
  const size_t step = (size_t)1 << (top - 3);
  return (bytes + step - 1) & ~(step - 1);
}

static hipError_t block_take(size_t bytes, void **out)
{
  if (t_pool)
  {
    auto it = t_pool->idle.find(bytes);
    if (it != t_pool->idle.end())
    {
      *out = it->second;
      t_pool->idle_bytes -= it->first;
      t_pool->live_bytes += bytes;
      t_pool->idle.erase(it);
      return hipSuccess;
    }
  }
  hipError_t e = hipMalloc(out, bytes);
  if (e == hipErrorOutOfMemory && t_pool && !t_pool->idle.empty())
  {
    (void)hipGetLastError();
    t_pool->trim(0);
    e = hipMalloc(out, bytes);
  }
  if (e == hipSuccess && t_pool) t_pool->live_bytes += bytes;
  return e;
}

static void block_give(void *p, size_t bytes)
{
  if (!t_pool)
  {
    (void)hipFree(p);
    return;
  }
  t_pool->idle.emplace(bytes, p);
  t_pool->idle_bytes += bytes;
  t_pool->live_bytes -= std::min(bytes, t_pool->live_bytes);
  const size_t cap = std::min(kPoolIdleMax, std::max(kPoolIdleMin, t_pool->live_bytes / 4u));
  if (t_pool->idle_bytes > cap) t_pool->trim(cap / 2u);
}

template <typename T>
struct DevBuf
{
  T *p = nullptr;
  size_t cap = 0; // elements
  int ensure(size_t n)
  {
    if (n <= cap) return 0;
    ++*t_epoch;
    if (p)
    {
      block_give(p, cap * sizeof(T)); // (its readers and writers so far are ahead of the next owner's on the stream)
      p = nullptr;
      cap = 0;
    }
    const size_t bytes = block_bytes(n * sizeof(T));
    void *q = nullptr;
    HIP_TRY(block_take(bytes, &q));
    p = static_cast<T *>(q);
    cap = bytes / sizeof(T);
    return 0;
  }
  void release()
  {
    if (p)
    {
      block_give(p, cap * sizeof(T));
      ++*t_epoch;
    }
    p = nullptr;
    cap = 0;
  }
};

// mapped result block: [0..7] lnL / derivative words, [8..) ascertainment-bias terms (up to 64 x 4 doubles)
constexpr size_t kResultBytes = (8 + 4 * 64) * sizeof(double);
constexpr unsigned kAscOff = 8;
constexpr unsigned kRepHostCap = 1u << 16; // ops of one class-map call whose counts the mapped block holds (larger calls go in pieces)
constexpr unsigned char kMap8 = 1, kMap32 = 2;

// replicate weights drawn on the device (kernels_rell.h): the prefix sums of the pattern weights, then {total, sites of
// weight != 1}; stale after every pllgpu_pattern_weights_upload. Outside resample_bytes: 8 x sites + 16 bytes of its own
struct RellState
{
  DevBuf<unsigned long long> cdf;
  bool stale = true;
  unsigned long long total = 0, not_one = 0;
};

constexpr unsigned kMaxPending = 56; // ops a tree launch may leave unstored (pllgpu_ctx::pending): eight seven-op groups, 32 of them tip x tip

struct pllgpu_ctx
{
  unsigned long long alloc_epoch = 1; // moves whenever one of this context's device blocks is (re)allocated or freed
  BlockPool pool;                     // device blocks this context has let go of (DevBuf)
  pllgpu_geometry_t geo;
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;

  // derived kernel geometry
  GenGeo gg;
  int ich = 0;
  bool dna_fast = false;
  bool use_mfma = false;
  int mfma_ng = 16;         // 4-state groups the MFMA kernels run with: 16 (33..64 states), 8 (21..32), 5 (17..20)
  unsigned mfma_wide = 1;   // 33..64 states, inner x inner: k_partials_mfma_wide (kernels_mfma_wide.h); PLL_AMD_MFMA_WIDE=0 (A/B, parity tests): k_partials_mfma
  bool mfma_pad = false;    // PLL_AMD_MFMA_PAD=1 (A/B): 61 states through the padded 64-state contraction
  unsigned xcd_order = 1;   // PLL_AMD_NO_XCD_ORDER=1 (A/B): store-bound launches in the natural workgroup order (kernels_common.h: xcd_block)
  bool tiled = false;       // generic shapes keep CLVs in the tiled sites-contiguous layout
  DevBuf<double> scratch;   // host-layout staging for mirror copies of tiled CLVs
  size_t pm_stride = 0; // doubles per matrix in PT layout
  unsigned span = 0;

  std::vector<DevBuf<double>> clv;
  std::vector<unsigned char> clv_aos;   // 4x4: the node's device CLV is entry-contiguous (class-compressed node)
  std::vector<DevBuf<unsigned>> scaler;
  std::vector<DevBuf<unsigned char>> tipchars;
  std::vector<DevBuf<unsigned>> site_id, id_site;
  std::vector<DevBuf<unsigned char>> site_id8; // site -> class in bytes: nodes with <= kRepNarrow classes (kernels_repeats.h)
  std::vector<unsigned char> map_forms;        // per node: which forms of its site -> class map are current (kMap8 | kMap32)
  std::vector<DevBuf<unsigned>> lent, rent; // class -> child entry, per compressed node (kernels_repeats.h)
  std::vector<int> rep_left, rep_right;     // the children those maps were built for, or -1
  std::vector<unsigned> ids;
  DevBuf<unsigned long long> tipmap;
  bool tipmap_set = false;
  DevBuf<double> pmat, freqs, rate_weights, prop_invar, persite, block_sums;
  DevBuf<double> edge_partials;   // k_edge_mfma: [rate][row group][site] partial site likelihoods
  DevBuf<unsigned> edge_tickets;  // ... and the ticket per item block (zero between launches)
  DevBuf<unsigned> counter;
  // pllgpu_insertion_loglikelihoods (kernels_insertion.h): [candidate][workgroup] partial sums, a ticket per candidate
  // (zero between launches), the results of a whole call, the candidates' descriptors of one launch
  DevBuf<double> ins_partials, ins_results;
  DevBuf<unsigned> ins_tickets;
  DevBuf<unsigned char> ins_cands;
  // pllgpu_placement_loglikelihoods (kernels_placement.h) uses the four above - slots and tickets per (query, candidate)
  // of a launch, the [query][candidate] results of a call - and the code rows of the call's queries
  DevBuf<unsigned char> plc_rows;
  // pllgpu_quartet_resampled_loglikelihoods (kernels_resample.h): per-site values [value][sites padded], their weighted form
  // [value][sites], the replicates' weights [replicate][sites padded to 4], partials [split][value][replicate], results
  // [value][replicate] - of one chunk each, together at most resample_bytes (PLLGPU_RESAMPLE_MAX_BYTES; PLL_AMD_RESAMPLE_SCRATCH lowers it)
  DevBuf<double> rs_u, rs_weighted, rs_part, rs_out;
  DevBuf<unsigned> rs_w;
  size_t resample_bytes = PLLGPU_RESAMPLE_MAX_BYTES;
  hipEvent_t rs_ev[4] = {nullptr, nullptr, nullptr, nullptr}; // around the upload, stage 1 and stage 2 of a call's first chunk
  double rs_ms[3] = {0.0, 0.0, 0.0};
  // replicate weights drawn on the device (kernels_rell.h): made by the first draw - a context that never draws carries
  // the pointer and nothing else
  RellState *rell = nullptr;
  DevBuf<unsigned char> mfma_flags;      // [op in launch][rate][entry] scaling decisions (kernels_mfma.h)
  DevBuf<double> eigenvals, rates, diag; // derivatives: [rate_matrices][SP], [R], [R][S][4]
  DevBuf<double> newton;                 // pllgpu_optimize_branch_length: the state record (NewtonState), then the trace
  unsigned newton_batch = 8;             // ... and how many evaluations it enqueues between two polls (tools/newton_device_latency.py)
  unsigned distance_pairs = PLLGPU_DISTANCE_MAX_PAIRS; // pllgpu_pairwise_distances: cells of the pair matrix per launch; PLL_AMD_DISTANCE_PAIRS lowers it (tests)
  size_t bootstrap_bytes = PLLGPU_BOOTSTRAP_MAX_BYTES; // pllgpu_bootstrap_distance_trees: device bytes of a chunk of replicates; PLL_AMD_BOOTSTRAP_BYTES lowers it (tests)
  double bs_ms[3] = {0.0, 0.0, 0.0};     // ... and its first chunk's draw, distance launches and join, by stream events (rs_ev)
  unsigned rell_range = kRellRange;      // k_rell_draw's sites per workgroup; PLL_AMD_RELL_RANGE lowers it (tests: a small case over several ranges)
  DevBuf<double> evecs, ievecs, brlen;   // device P-matrices: [rate_matrices][S][SP] x 2, staged branch lengths
  DevBuf<unsigned> mindex;               // staged matrix indices
  DevBuf<unsigned> rep_table, rep_blocksum, rep_counts; // site-repeats class computation (kernels_repeats.h): arena, bitmaps, counts per op of a call
  DevBuf<unsigned> rep_sync;             // [kRepOps] tickets per op of a launch, then the launch's own (zero between launches)
  DevBuf<unsigned char> rep_ops;         // the op descriptors of one call
  std::vector<RepOp> rep_ops_host;
  unsigned rep_wgs = 0;                  // PLL_AMD_REP_WGS: workgroups per op of k_rep_mark (0: by the launch's size)
  unsigned rep_max_ranges = 8;           // PLL_AMD_REP_RANGES: site ranges per part of a large table, at most (kernels_repeats.h)
  bool sub_pack_always = false;          // PLL_AMD_SUB_PACK_ALWAYS=1: k_sub_pack after every class-map call, whatever it reported (A/B)
  bool rep_bits = true;                  // PLL_AMD_REP_BITS=0: the bitmap of first sites by atomics + k_rep_scan for every table size (A/B)
  bool rep_hints = true;                 // PLL_AMD_REP_HINTS=0: every level of a class-map call is launched (A/B, tests)
  unsigned long long rep_hint_key = 0;   // the last call: a hash of its (parent, left, right, level) records ...
  unsigned rep_hint_count = 0, rep_hint_level = 0; // ... their number, the highest level with a compressed parent ...
  bool rep_hint_any = false;                       // ... if there was one
  bool rep_scratch_dirty = false;        // a class-map call did not complete: its bitmaps and tickets are cleared before the next
  DevBuf<double> sumtable[PLLGPU_SUMTABLE_SLOTS]; // device-resident sumtables (tiled like a CLV), allocated on first use
  double *result_dev = nullptr;  // device alias of result_host
  DevBuf<unsigned> pattern_weights;
  DevBuf<int> invariant;
  bool invariant_set = false;
  unsigned *rep_host = nullptr;  // pinned + mapped: class counts of a class-map call [rep_host_cap], the sequence word, an error word
  unsigned *rep_host_dev = nullptr;
  unsigned rep_host_cap = 0;
  unsigned rep_seq = 0;
  double *result_host = nullptr; // pinned + mapped: [0] lnL, [1] sequence of the call that wrote it
  double seq = 0.0;
  double seq_override = 0.0;     // pllgpu_edge_t.sequence of the evaluation being issued (0: number it here)
  DevBuf<double> reduce;         // {lnL, sequence}: the operand of a caller's all-reduce (pllgpu_reduce_buffer)
  DevBuf<double> ancestral;      // [sites][states] staging of pllgpu_node_ancestral's host output, allocated on first use
  // pllgpu_edge_category_posteriors / pllgpu_category_weights_em (kernels_category.h): the table [R][sites padded to 64],
  // the count word per site, partials [R + 1][B], results [evaluation][R + 1], the EM call's weight rows [steps + 1][R],
  // and the staging of the three per-site outputs - each allocated on first use
  DevBuf<double> cat_table, cat_partials, cat_results, cat_weights, cat_lnl, cat_posterior, cat_rates;
  DevBuf<unsigned> cat_count;
  std::vector<double> stage;     // host staging for the P-matrix re-layout
  std::vector<unsigned char> stage8; // ... and for a class map that goes up as bytes
  unsigned last_launches = 0;
  unsigned long long rep_ops_total = 0, rep_launches_total = 0; // class-map ops handed to the device / class kernels launched, ever
  unsigned long long rep_calls_total = 0;                       // pllgpu_repeats_classes calls served (a repeat after a wrong forecast is none)
  double last_bytes = 0.0;       // algorithmic HBM bytes of the last update_partials call
  bool no_tip_columns = false;   // PLL_AMD_NO_TIP_COLUMNS=1: tips always through the FMA contraction
  bool tt_stream = true;         // PLL_AMD_TT_STREAM=0: plain tip x tip levels of 33..64 states through k_partials_mfma's column route (round 5) - the control
  bool no_par_lds = false;       // PLL_AMD_NO_PARENT_LDS=1 (A/B): entry-contiguous parents stored 8 bytes per lane
  bool no_coop_fetch = false;    // PLL_AMD_NO_COOP_FETCH=1 (A/B): the FMA kernels' entry-contiguous children fetched per lane
  size_t stream_parent_bytes = (size_t)256 << 20; // parents of a grouped launch beyond this leave with streaming stores (the Infinity Cache)
  bool defer_tail = false;       // DNA: hold the traversal's last ops for one call (k_edge_dna_tail)
  std::vector<pllgpu_op_t> deferred; // ops accepted by pllgpu_update_partials and not launched yet
  bool fuse_cc = false;          // DNA: also two producer levels under a group parent (cherry-cherry children)
  int fuse_cc16 = -1;            // DNA, chain plans: also a parent over two complete 8-tip groups (fifteen ops, k_partials_dna_cc16):
                                 // -1 by size (chain_plan.h: use_cc16), 0 never, 1 always (PLL_AMD_FUSE_CC16)
  int fuse_tree = -1;            // DNA, chain plans: a balanced 64-taxon traversal and its edge evaluation as one launch (k_edge_dna_tree):
                                 // -1 by size (chain_plan.h: use_tree), 0 never, 1 always (PLL_AMD_FUSE_TREE)
  bool fuse_gg = true;           // DNA + site repeats: groups over two gathering producers (PLL_AMD_NO_FUSE_GG=1: off)
  bool fuse = false;             // DNA: evaluate producer + consumer ops in one kernel (kernels_dna.h)
  bool chains = false;           // DNA: chain plans (k_partials_dna_chain) for dependency-only op lists
  bool any_aos = false;          // a class-compressed CLV exists (site repeats): no chain plans
  struct ChainPlan *plan = nullptr; // the last chain plan, re-launched as is when the same list comes again
  bool chain_held = false;          // the plan's last stage has not been launched yet (chain tail, kernels_dna.h)
  bool tree_held = false;           // ... and neither has its stage 1: the whole plan waits (ChainPlan::tree; implies chain_held)
  // Lazy cherries: the whole-traversal launch ran in its lean form (k_edge_dna_tree<NoCherries>) and did not store the list's 32
  // tip x tip parents. They are PENDING: a representation, not work in flight - each is a function of two tip code vectors
  // and two matrices that are on the device and have not changed since (every entry point that could read a pending CLV or
  // scaler, overwrite it or change one of its inputs stores them first: materialise_pending). Never non-empty while
  // anything is held: the launch that leaves them consumed the held plan, and the next update call resolves them.
  // A matrix one of them reads may change all the same (the model-parameter loop rewrites every matrix between two steps,
  // a branch-length pass the evaluated edge's): the 64 matrices of the step are copied aside first, device to device in
  // one small launch (keep_pending_matrices), and the pending ops are stored from the copies if they are stored at all.
  // Lazy subtrees: inside a loop that reads no CLV between its steps (the plan's own list again while its ops are still
  // pending) the launch runs in its deep form and stores nothing of the eight 8-tip groups: 56 ops pending, 112 matrices.
  bool lazy_cherries = true;          // PLL_AMD_LAZY_CHERRIES=0: the launch stores everything
  int lazy_subtrees = -1;             // PLL_AMD_LAZY_SUBTREES: the deep form -1 by size (chain_plan.h: use_deep_tree), 0 never, 1 at any size
  bool tree_deep = false;             // the held whole traversal, if evaluated in one launch, takes the deep form (set by every update call)
  std::vector<pllgpu_op_t> pending;   // the ops as planned: parent CLV, scaler, tip and matrix indices - the 32 tip x tip ops,
                                      // or the 56 group ops in group order (ChainPlan::subtrees)
  bool pending_deep = false;          // ... the latter: stored by one seven-op group launch
  const struct ChainPlan *pending_plan = nullptr; // the plan they belong to: its own list again recomputes them all
  DevBuf<double> pending_mats;        // op i's left and right matrix as they were at the step: slots 2i, 2i + 1 ...
  bool pending_mats_kept = false;     // ... once one of them was about to change (else the ops read c->pmat)
  DevBuf<unsigned char> chain_dev;  // its descriptors
  // level-scheduled lists: the launches of a planned list are kept (descriptor packs by value) and replayed
  // as they are when the same list comes again while nothing they point at has moved (LevelPlan below)
  unsigned long long maps_epoch = 1; // bumped whenever the SHAPE of the class maps changes: a node's class count, the children its entry maps
                                     // were built for, the form of its site -> class map (cached launches carry counts and pointers)
  unsigned long long maps_version = 1; // bumped whenever class maps are written at all (data derived from their CONTENTS: k_sub_pack)
  std::vector<unsigned char> map_widened; // per node: a launch reads the 32-bit form although the class kernels write bytes (wide_map)
  std::vector<struct LevelPlan *> level_plans;
  struct LevelPlan *recording = nullptr;
  int launch_rc = 0;                // a launch helper that failed inside emit_launch()
  int fenced = 0;                   // PLL_AMD_FENCED_HANDOFF=1 (kernels_common.h: handoff_*)
  unsigned long long plan_stamp = 0;
  unsigned long long plan_replays = 0; // op lists that were launched from a kept plan (chain or level), ever
  bool plan_cache = true;           // PLL_AMD_NO_PLAN_CACHE=1 plans every call afresh
  DevBuf<unsigned char> cherry_bits; // k_cherry_bits: which cherry entries are rescaled, [slot][rate][pair of tip codes]
  struct CherrySlot
  {
    unsigned long long lver = 0, rver = 0, maps = 0;
  };
  std::map<unsigned long long, unsigned> cherry_slot_of; // (left matrix, right matrix) -> slot
  std::vector<CherrySlot> cherry_slot;                   // what the slot's table was computed from
  std::vector<unsigned long long> pm_version;            // bumped whenever a device matrix is written
  unsigned tip_ncodes = 0;          // codes in use: 1 + the highest code with a non-empty mask
  bool generic_aos = true;          // PLL_AMD_NO_GENERIC_AOS=1: compressed nodes of non-4x4 shapes stay tiled (A/B)
  bool lean = false;                // 17..20 states, <= 4 rates: the level launches on the matrix pipe (kernels_lean.h)
  bool fuse_mfma = false;           // 17..32 states on the matrix pipe: the same groups (kernels_mfma.h: k_partials_mfma_cc)
  bool subtrees = false;            // DNA + site repeats: all-tip subtrees straight from the tip codes (subtree_plan.h)
  DevBuf<unsigned char> sub_dev;    // their descriptors on the device ...
  std::vector<SubItem> sub_cache, sub_build; // ... and what that array holds / the list being planned
  unsigned long long sub_epoch = 0;
  DevBuf<unsigned long long> sub_packed; // k_sub_pack: per sub-tree op and entry, the tip codes below it
  bool sub_pack_valid = false;           // ... formed for the descriptors on the device, the class maps (maps_version) ...
  unsigned long long sub_pack_maps = 0, sub_pack_tips = 0, tips_epoch = 1; // ... and the tip data (tips_epoch) of now
  unsigned long long maps_foreign = 1, sub_pack_foreign = 0; // maps written by anything but the class kernels (uploads, count changes)
  unsigned sub_pack_since = 0;           // the class-map calls from this sequence number on came after the packed words
  DevBuf<unsigned> rep_changed;          // RepPack::changed
  std::vector<DevBuf<unsigned>> rep_keep; // per node: RepOp::keep
  std::vector<unsigned char> rep_ops_sent; // the descriptors the device array holds (bytes), and where
  const void *rep_ops_sent_at = nullptr;
  DevBuf<unsigned> rep_final;            // RepOp::final of the deferred ops of a call (kRepFuseCells cells each)
  bool rep_fuse = true;                  // PLL_AMD_REP_FUSE=0: every op's site -> class pass in k_rep_assign (A/B)
  // small transfers go through one block of pinned, device-visible host memory (stage_take below)
  unsigned char *ring_host = nullptr, *ring_dev = nullptr;
  size_t ring_cap = 0, ring_off = 0;
  bool ring_failed = false;
  // downloads through the block that have been enqueued but not waited for (pllgpu_download_defer)
  struct PendingDown
  {
    void *host;
    const unsigned char *ring;
    size_t bytes;
  };
  std::vector<PendingDown> pending_down;
  bool defer_down = false;
};

// what pllgpu_update_partials did for one op list through the level scheduler: its launches, in order, with
// their descriptor packs captured by value; the ops it held back for the log-likelihood kernel; the CLV layout
// flags resolve_op() left behind. Valid while no device block has been (re)allocated (pllgpu_ctx::alloc_epoch) and no
// class map has changed (maps_epoch).
struct LevelPlan
{
  std::vector<pllgpu_op_t> key;
  unsigned long long alloc_epoch = 0, maps_epoch = 0;
  std::vector<std::function<int()>> launches; // each returns 0 or the error of its launcher
  std::vector<pllgpu_op_t> deferred;
  std::vector<std::pair<unsigned, unsigned char>> aos; // (node, entry-contiguous?) as the list leaves them
  unsigned nlaunches = 0;
  double bytes = 0.0;
  bool any_aos = false;
  unsigned long long used = 0; // LRU stamp
};
constexpr size_t kLevelPlans = 4;

// the one way the level scheduler launches: run `launch` now and, while a plan is being recorded, keep it for the
// replays. Its error, if any, stays in launch_rc (a replay leaves it there as well); `count` = the launches it stands
// for in pllgpu_last_launch_count. Returns launch_rc.
template <class F>
static inline int emit_launch(pllgpu_ctx *c, F &&launch, unsigned count = 1)
{
  if (int rc = launch()) c->launch_rc = rc;
  if (c->recording) c->recording->launches.emplace_back(std::forward<F>(launch));
  c->last_launches += count;
  return c->launch_rc;
}

static inline int use(pllgpu_ctx *c)
{
  HIP_TRY(hipSetDevice(c->device));
  return 0;
}

// Every entry point works on the context's device and leaves the calling thread's current HIP device as it
// found it (the thread may belong to torch or to another HIP user with a different device selected).
struct DeviceScope
{
  int prev = -1, rc = 0;
  unsigned long long *prev_epoch;
  BlockPool *prev_pool;
  explicit DeviceScope(pllgpu_ctx *c) : prev_epoch(t_epoch), prev_pool(t_pool)
  {
    t_epoch = &c->alloc_epoch; // whose blocks this entry point may move (entry points nest: put back on the way out)
    t_pool = &c->pool;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != c->device) rc = use(c);
    else prev = -1; // nothing to restore
  }
  ~DeviceScope()
  {
    t_epoch = prev_epoch;
    t_pool = prev_pool;
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// hipFuncSetAttribute applies to the CURRENT device: once per (kernel, device), not once per process
static void raise_lds_limit(const void *fn, int device, size_t dynamic_bytes)
{
  // dynamic LDS beyond the default limit has to be announced per kernel; the kernel's static LDS counts
  // against the 160 KB as well, so only what a launch needs is asked for (the largest request so far)
  static std::mutex mu;
  static std::map<std::pair<const void *, int>, size_t> done;
  std::lock_guard<std::mutex> g(mu);
  size_t &have = done[{fn, device}];
  if (dynamic_bytes <= have || dynamic_bytes <= 32 * 1024) return;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dynamic_bytes) != hipSuccess)
    (void)hipGetLastError(); // the launch itself will report what is wrong
  else
    have = dynamic_bytes;
}

extern "C" const char *pllgpu_last_error(void) { return g_err; }

extern "C" int pllgpu_device_count(void)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

extern "C" int pllgpu_default_device(void)
{
  const char *env = getenv("PLL_AMD_DEVICE");
  int device = 0;
  if (env && strcmp(env, "auto") == 0) return -2;
  if (env) return atoi(env);
  if (hipGetDevice(&device) != hipSuccess)
  {
    (void)hipGetLastError();
    device = 0;
  }
  return device;
}

extern "C" int pllgpu_context_device(const pllgpu_ctx_t *c) { return c ? c->device : -1; }

static void derive_geometry(pllgpu_ctx *c)
{
  const pllgpu_geometry_t &g = c->geo;
  int ich = g.states <= 4 ? 4 : g.states <= 8 ? 8 : g.states <= 16 ? 16 : g.states <= 20 ? 20 : 32;
  GenGeo &gg = c->gg;
  gg.S = g.states;
  gg.SP = g.states_padded;
  gg.R = g.rate_cats;
  gg.nchunks = (g.states + ich - 1) / ich;
  gg.SPT = gg.nchunks * ich;
  gg.tile_sz = g.rate_cats * g.states * 64u;
  gg.scale_mode = g.per_rate_scalers ? 2 : 1;
  c->ich = ich;
  c->dna_fast = (g.states == 4 && g.rate_cats == 4);
  if (const char *v = getenv("PLL_AMD_GENERIC_ONLY")) // experiment switch: route DNA through the generic kernels
    if (*v && *v != '0') c->dna_fast = false;
  c->fuse = c->dna_fast;
  if (const char *v = getenv("PLL_AMD_NO_FUSE")) // experiment switch: one kernel per op group, no producer/consumer fusion
    if (*v && *v != '0') c->fuse = false;
  if (const char *v = getenv("PLL_AMD_TT_STREAM")) c->tt_stream = !(*v == '0');
  if (const char *v = getenv("PLL_AMD_NO_TIP_COLUMNS"))
    if (*v && *v != '0') c->no_tip_columns = true;
  if (const char *v = getenv("PLL_AMD_NO_PARENT_LDS"))
    if (*v && *v != '0') c->no_par_lds = true;
  if (const char *v = getenv("PLL_AMD_NO_COOP_FETCH"))
    if (*v && *v != '0') c->no_coop_fetch = true;
  c->defer_tail = c->dna_fast;
  if (const char *v = getenv("PLL_AMD_NO_TAIL_FUSION"))
    if (*v && *v != '0') c->defer_tail = false;
  c->fuse_cc = c->fuse;
  c->fuse_cc16 = -1;
  if (const char *v16 = getenv("PLL_AMD_FUSE_CC16"))
    if (*v16) c->fuse_cc16 = *v16 != '0' ? 1 : 0;
  c->fuse_tree = -1;
  if (const char *vt = getenv("PLL_AMD_FUSE_TREE"))
    if (*vt) c->fuse_tree = *vt != '0' ? 1 : 0;
  c->lazy_cherries = true;
  if (const char *v = getenv("PLL_AMD_LAZY_CHERRIES"))
    if (*v) c->lazy_cherries = *v != '0';
  c->lazy_subtrees = -1;
  if (const char *v = getenv("PLL_AMD_LAZY_SUBTREES"))
    if (*v) c->lazy_subtrees = *v != '0' ? 1 : 0;
  if (const char *v = getenv("PLL_AMD_NO_FUSE_CC"))
    if (*v && *v != '0') c->fuse_cc = false;
  c->chains = c->fuse;
  if (const char *v = getenv("PLL_AMD_NO_CHAINS"))
    if (*v && *v != '0') c->chains = false;
  if (const char *v = getenv("PLL_AMD_NO_GENERIC_AOS"))
    if (*v && *v != '0') c->generic_aos = false;
  if (const char *v = getenv("PLL_AMD_FENCED_HANDOFF"))
    if (*v && *v != '0') c->fenced = 1;
  if (const char *v = getenv("PLL_AMD_NO_PLAN_CACHE"))
    if (*v && *v != '0') c->plan_cache = false;
  if (const char *v = getenv("PLL_AMD_NEWTON_BATCH")) // A/B (tools/newton_device_latency.py): evaluations enqueued per host wait
    if (atoi(v) >= 1) c->newton_batch = (unsigned)std::min(atoi(v), PLLGPU_NEWTON_MAX_ITERS);
  if (const char *v = getenv("PLL_AMD_NO_FUSE_GG"))
    if (*v && *v != '0') c->fuse_gg = false;
  if (const char *v = getenv("PLL_AMD_RESAMPLE_SCRATCH")) // tests: bytes of scratch the resampling call may use, so that a tiny case is cut
    if (atoll(v) >= 1) c->resample_bytes = std::min<size_t>((size_t)atoll(v), PLLGPU_RESAMPLE_MAX_BYTES);
  if (const char *v = getenv("PLL_AMD_RELL_RANGE")) // tests: sites per workgroup of k_rell_draw, a multiple of 4
    if (atoll(v) >= 4) c->rell_range = (unsigned)std::min<long long>(atoll(v) / 4 * 4, kRellRange);
  if (const char *v = getenv("PLL_AMD_DISTANCE_PAIRS")) // tests: a small list over several launches
    if (atoll(v) >= 1) c->distance_pairs = (unsigned)std::min<long long>(atoll(v), PLLGPU_DISTANCE_MAX_PAIRS);
  if (const char *v = getenv("PLL_AMD_BOOTSTRAP_BYTES")) // tests: a few replicates over several chunks
    if (atoll(v) >= 1) c->bootstrap_bytes = std::min<size_t>((size_t)atoll(v), PLLGPU_BOOTSTRAP_MAX_BYTES);
  c->subtrees = c->dna_fast;
  if (const char *v = getenv("PLL_AMD_NO_SUBTREES")) // A/B switch: the bottom levels under site repeats go level by level
    if (*v && *v != '0') c->subtrees = false;
  c->tiled = true; // every shape keeps CLVs in the tiled sites-contiguous layout
  // 33..64 states: CLV updates on the fp64 matrix pipe (kernels_mfma.h); PLL_AMD_NO_MFMA=1 keeps the FMA kernel
  {
    // PLL_AMD_MFMA_MIN_STATES: from how many states on the CLV updates run on the matrix pipe
    unsigned min_states = 33;
    if (const char *v = getenv("PLL_AMD_MFMA_MIN_STATES")) min_states = (unsigned)std::max(17, atoi(v));
    c->use_mfma = (g.states >= min_states && g.rate_cats <= 16);
    c->mfma_ng = g.states > 32 ? 16 : g.states > 20 ? 8 : 5;
  }
  if (const char *v = getenv("PLL_AMD_NO_MFMA"))
    if (*v && *v != '0') c->use_mfma = false;
  if (const char *v = getenv("PLL_AMD_MFMA_WIDE")) c->mfma_wide = atoi(v) != 0 ? 1u : 0u;
  if (const char *v = getenv("PLL_AMD_MFMA_PAD")) c->mfma_pad = *v && *v != '0';
  if (const char *v = getenv("PLL_AMD_NO_XCD_ORDER")) c->xcd_order = (*v && *v != '0') ? 0u : 1u;
  // (tip x tip, tip x tip -> inner x inner) groups of 17..32 states: on the matrix pipe (kernels_mfma.h:
  // k_partials_mfma_cc), whatever pipe the level launches use - C3 (20 states) 4.0 -> 5.1 G updates/s on the same box
  // (profiles/README.md, round 2). PLL_AMD_FUSE_GENERIC=0 or PLL_AMD_NO_FUSE=1: level launches only (A/B, parity tests).
  // (The table-fed FMA groups, the 33..64-state groups and the inner x inner groups of rounds 1-2 measured slower than
  // the launches they replaced and are gone; their numbers stay in profiles/README.md.)
  bool groups = true;
  if (const char *v = getenv("PLL_AMD_FUSE_GENERIC")) groups = *v && *v != '0';
  if (const char *v = getenv("PLL_AMD_NO_FUSE"))
    if (*v && *v != '0') groups = false;
  c->fuse_mfma = groups && g.rate_cats <= 16 && g.states >= 17 && g.states <= 32;
  c->lean = !c->dna_fast && !c->use_mfma && g.states >= 17 && g.states <= 20 && g.rate_cats <= 4;
  if (const char *v = getenv("PLL_AMD_NO_LEAN")) // A/B switch: the scalar-fed FMA kernels for these shapes
    if (*v && *v != '0') c->lean = false;
  c->pm_stride = (size_t)g.rate_cats * g.states * gg.SPT;
  c->span = g.rate_cats * g.states_padded;
}

// A node that holds fewer entries than sites is class-compressed (site repeats): its CLV stays
// entry-contiguous on the device, in the host's own layout [entry][rate][states_padded] - gathers then read
// whole entries (kernels_dna.h, kernels_generic.h). The matrix-pipe kernels (33..64 states) keep the tiled layout.
static inline bool aos_entries(const pllgpu_ctx *c, unsigned entries)
{
  return (c->dna_fast || (c->generic_aos && !c->use_mfma)) && entries != c->geo.sites_alloc;
}

// doubles of device storage for `entries` entries of one CLV
static inline size_t clv_elems(const pllgpu_ctx *c, unsigned entries)
{
  if (aos_entries(c, entries)) return (size_t)entries * c->span;
  if (c->tiled) return (size_t)((entries + 63u) / 64u) * c->gg.tile_sz;
  return (size_t)entries * c->span;
}

// the device a new context or parsimony record lands on (device < 0: PLL_AMD_DEVICE, or the calling thread's current
// device), checked to be a gfx950; -1 with the error set
static int pick_device(int device)
{
  int n = pllgpu_device_count();
  if (n <= 0)
  {
    fail(PLLGPU_ENODEVICE, "no HIP device visible (hipGetDeviceCount = %d)", n);
    return -1;
  }
  if (device < 0)
  {
    // PLL_AMD_DEVICE=<n>: that device; PLL_AMD_DEVICE=auto: new partitions go round-robin over the visible
    // devices (thread-per-partition callers such as RAxML-NG use every GPU of the node without a code change);
    // unset: the calling thread's current HIP device
    const char *env = getenv("PLL_AMD_DEVICE");
    static std::atomic<unsigned> next_device{0};
    if (env && strcmp(env, "auto") == 0)
      device = (int)(next_device.fetch_add(1, std::memory_order_relaxed) % (unsigned)n);
    else if (env)
      device = atoi(env);
    else if (hipGetDevice(&device) != hipSuccess)
      device = 0;
  }
  if (device >= n)
  {
    fail(PLLGPU_EINVAL, "device %d out of range (%d visible)", device, n);
    return -1;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess)
  {
    fail(PLLGPU_ENODEVICE, "hipGetDeviceProperties(%d) failed", device);
    return -1;
  }
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
  {
    fail(PLLGPU_ENODEVICE, "device %d is %s; this library carries gfx950 (MI355X) code only", device,
         prop.gcnArchName);
    return -1;
  }
  return device;
}

extern "C" pllgpu_ctx_t *pllgpu_create(const pllgpu_geometry_t *geo, int device)
{
  device = pick_device(device);
  if (device < 0) return nullptr;
  if (geo->states < 2 || geo->states > 64 || geo->rate_cats < 1 || geo->rate_cats > (unsigned)kMaxRates)
  {
    fail(PLLGPU_EUNSUPPORTED, "unsupported shape: states=%u (2..64) rate_cats=%u (1..%d)", geo->states,
         geo->rate_cats, kMaxRates);
    return nullptr;
  }
  pllgpu_ctx *c = new pllgpu_ctx();
  c->geo = *geo;
  c->device = device;
  derive_geometry(c);
  DeviceScope device_scope_(c); // the caller's current device comes back when this function returns
  bool ok = device_scope_.rc == 0 && hipSetDevice(device) == hipSuccess &&
            hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess &&
            hipEventCreate(&c->ev0) == hipSuccess && hipEventCreate(&c->ev1) == hipSuccess &&
            hipHostMalloc((void **)&c->result_host, kResultBytes, hipHostMallocMapped) == hipSuccess &&
            hipHostGetDevicePointer((void **)&c->result_dev, c->result_host, 0) == hipSuccess &&
            hipHostMalloc((void **)&c->rep_host, (kRepHostCap + 2) * sizeof(unsigned), hipHostMallocMapped) == hipSuccess &&
            hipHostGetDevicePointer((void **)&c->rep_host_dev, c->rep_host, 0) == hipSuccess;
  c->rep_host_cap = kRepHostCap;
  if (!ok)
  {
    fail(PLLGPU_ERUNTIME, "stream/event creation failed: %s", hipGetErrorString(hipGetLastError()));
    pllgpu_destroy(c);
    return nullptr;
  }
  c->own_stream = true;
  memset(c->result_host, 0, 8 * sizeof(double));
  memset(c->rep_host, 0, (kRepHostCap + 2) * sizeof(unsigned));
  c->clv.resize(geo->nodes);
  c->clv_aos.assign(geo->nodes, 0);
  c->scaler.resize(geo->scale_buffers);
  c->tipchars.resize(geo->tips);
  c->site_id.resize(geo->nodes);
  c->id_site.resize(geo->nodes);
  c->site_id8.resize(geo->nodes);
  c->rep_keep.resize(geo->nodes);
  c->map_forms.assign(geo->nodes, 0);
  c->map_widened.assign(geo->nodes, 0);
  c->lent.resize(geo->nodes);
  c->rent.resize(geo->nodes);
  c->rep_left.assign(geo->nodes, -1);
  c->rep_right.assign(geo->nodes, -1);
  c->ids.assign(geo->nodes, 0);
  if (c->pmat.ensure(c->pm_stride * (geo->prob_matrices + 2)) || c->freqs.ensure((size_t)geo->rate_matrices * geo->states_padded) ||
      c->rate_weights.ensure(geo->rate_cats) || c->prop_invar.ensure(geo->rate_matrices) ||
      c->pattern_weights.ensure(geo->sites_alloc) || c->persite.ensure(geo->sites_alloc) ||
      c->block_sums.ensure(4096) || c->counter.ensure(4) || (c->dna_fast && c->lazy_cherries && c->pending_mats.ensure(c->pm_stride * 2u * kMaxPending)) || c->rep_sync.ensure((size_t)kRepOps + 1) || c->rep_changed.ensure(1))
  {
    pllgpu_destroy(c);
    return nullptr;
  }
  (void)hipMemsetAsync(c->pmat.p, 0, c->pmat.cap * sizeof(double), c->stream);
  c->pm_version.assign(geo->prob_matrices + 2, 1ull);
  (void)hipMemsetAsync(c->prop_invar.p, 0, c->prop_invar.cap * sizeof(double), c->stream);
  (void)hipMemsetAsync(c->counter.p, 0, c->counter.cap * sizeof(unsigned), c->stream);
  (void)hipMemsetAsync(c->rep_sync.p, 0, c->rep_sync.cap * sizeof(unsigned), c->stream);
  (void)hipMemsetAsync(c->rep_changed.p, 0, sizeof(unsigned), c->stream);
  if (const char *v = getenv("PLL_AMD_REP_WGS")) c->rep_wgs = (unsigned)std::max(0, atoi(v));
  if (const char *v = getenv("PLL_AMD_REP_BITS")) c->rep_bits = !(*v == '0');
  if (const char *v = getenv("PLL_AMD_SUB_PACK_ALWAYS")) c->sub_pack_always = *v && *v != '0';
  if (const char *v = getenv("PLL_AMD_REP_FUSE")) c->rep_fuse = !(*v == '0');
  if (const char *v = getenv("PLL_AMD_PINNED_STAGING")) c->ring_failed = *v == '0'; // 0: every transfer from / to pageable memory as the runtime does it (A/B)
  if (const char *v = getenv("PLL_AMD_REP_HINTS")) c->rep_hints = !(*v == '0');
  if (const char *v = getenv("PLL_AMD_REP_RANGES")) c->rep_max_ranges = (unsigned)std::max(1, atoi(v));
  return c;
}

static void drop_chain_plan(pllgpu_ctx *c);

extern "C" void pllgpu_destroy(pllgpu_ctx_t *c)
{
  if (!c) return;
  DeviceScope device_scope_(c);
  c->deferred.clear(); // results nobody will ask for
  c->chain_held = c->tree_held = false;
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  drop_chain_plan(c);
  for (LevelPlan *lp : c->level_plans) delete lp;
  c->level_plans.clear();
  c->chain_dev.release();
  c->sub_dev.release();
  c->sub_packed.release();
  c->cherry_bits.release();
  c->pending_mats.release();
  for (auto &b : c->clv) b.release();
  for (auto &b : c->scaler) b.release();
  for (auto &b : c->tipchars) b.release();
  for (auto &b : c->site_id) b.release();
  for (auto &b : c->id_site) b.release();
  for (auto &b : c->site_id8) b.release();
  for (auto &b : c->rep_keep) b.release();
  for (auto &b : c->lent) b.release();
  for (auto &b : c->rent) b.release();
  c->tipmap.release();
  c->scratch.release();
  c->pmat.release();
  c->edge_partials.release();
  c->edge_tickets.release();
  c->ins_partials.release();
  c->ins_results.release();
  c->ins_tickets.release();
  c->ins_cands.release();
  c->rs_u.release();
  c->rs_weighted.release();
  c->rs_part.release();
  c->rs_out.release();
  c->rs_w.release();
  if (c->rell) c->rell->cdf.release();
  delete c->rell;
  for (hipEvent_t ev : c->rs_ev)
    if (ev) (void)hipEventDestroy(ev);
  c->freqs.release();
  c->rate_weights.release();
  c->prop_invar.release();
  c->persite.release();
  c->block_sums.release();
  c->reduce.release();
  c->ancestral.release();
  c->cat_table.release();
  c->cat_partials.release();
  c->cat_results.release();
  c->cat_weights.release();
  c->cat_lnl.release();
  c->cat_posterior.release();
  c->cat_rates.release();
  c->cat_count.release();
  c->counter.release();
  c->mfma_flags.release();
  c->eigenvals.release();
  c->evecs.release();
  c->ievecs.release();
  c->brlen.release();
  c->mindex.release();
  c->rep_table.release();
  c->rep_ops.release();
  c->rep_blocksum.release();
  c->rep_counts.release();
  c->rep_sync.release();
  c->rep_changed.release();
  c->rep_final.release();
  c->rates.release();
  c->diag.release();
  c->newton.release();
  for (auto &b : c->sumtable) b.release();
  c->pattern_weights.release();
  c->invariant.release();
  c->pool.trim(0); // everything above went to the context's idle blocks: back to the runtime now
  if (c->result_host) (void)hipHostFree(c->result_host);
  if (c->rep_host) (void)hipHostFree(c->rep_host);
  if (c->ring_host) (void)hipHostFree(c->ring_host);
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

// ---- data movement ---------------------------------------------------------------------------
// H2D copies from pageable caller memory: hipMemcpyAsync stages pageable sources before it
// returns, so the caller may reuse its buffer; ordering with kernels is by the stream.
// every entry point first launches what pllgpu_update_partials is holding back (tail fusion,
// kernels_dna.h) - except the edge evaluation, which may consume it
static int flush_deferred(pllgpu_ctx *c, bool keep_pending = false);
static int matrices_change(pllgpu_ctx *c, const unsigned *indices, unsigned first, unsigned count);
static int materialise_pending(pllgpu_ctx *c);
static void set_pending(pllgpu_ctx *c, const struct ChainPlan *pl, bool deep = false);
#define CHECK_CTX_KEEP(c)                    \
  if (!(c)) return fail(PLLGPU_EINVAL, "null context"); \
  DeviceScope device_scope_(c);              \
  if (device_scope_.rc) return device_scope_.rc
#define HOLDS_WORK(c) (!(c)->deferred.empty() || (c)->chain_held)
// ... and stores what the lean tree launch left unstored (pllgpu_ctx::pending): whoever comes through here may read it,
// overwrite it or change what it is a function of
#define CHECK_CTX(c)                                   \
  CHECK_CTX_KEEP(c);                                   \
  if (HOLDS_WORK(c) || !(c)->pending.empty())          \
    if (int rc_ = flush_deferred(c)) return rc_
// held work goes out, pending CLVs stay as they are: for calls that touch neither them nor their inputs (a held whole
// traversal goes out without the tip x tip stores too: chain_plan.h, launch_held_chains)
#define CHECK_CTX_KEEP_PENDING(c)                      \
  CHECK_CTX_KEEP(c);                                   \
  if (HOLDS_WORK(c))                                   \
    if (int rc_ = flush_deferred(c, true)) return rc_

// Small transfers. hipMemcpyAsync from or to pageable memory is a blocking trip through the runtime's own staging (10-25 us
// whatever the size; the flat pll_core_* seam made six of them per call): a transfer of up to kRingMax bytes goes through
// the context's block of pinned host memory instead - up: the caller's bytes are copied there and the device reads them
// from there (a copy enqueued from pinned memory, or the layout kernel straight out of host memory); down: the device
// writes there, one wait, the bytes are copied out. A piece of the block belongs to its transfer until the stream has
// been waited for; the block is handed out front to back and starts over after a wait (stream_wait).
constexpr size_t kRingCap = (size_t)8 << 20, kRingMax = (size_t)2 << 20;

// the stream has just been waited for: everything that read or wrote the block has completed
static void ring_drained(pllgpu_ctx *c)
{
  for (const auto &d : c->pending_down) memcpy(d.host, d.ring, d.bytes);
  c->pending_down.clear();
  c->ring_off = 0;
}

static hipError_t stream_wait(pllgpu_ctx *c)
{
  const hipError_t e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) ring_drained(c);
  else
  {
    // the downloads that were waiting for this did not happen: their host pointers (a caller's arrays, perhaps out of
    // scope by the next wait) are forgotten, and the block is not handed out again - what the device still does with
    // it is unknown
    c->pending_down.clear();
    c->ring_failed = true;
  }
  return e;
}

// `bytes` of the block: the host address, and the address the device knows the same memory by. nullptr: not this way
// (too large, or no pinned memory to be had) - the caller takes the pageable path.
static unsigned char *stage_take(pllgpu_ctx *c, size_t bytes, unsigned char **dev)
{
  if (bytes > kRingMax || c->ring_failed) return nullptr;
  if (!c->ring_host)
  {
    void *h = nullptr, *d = nullptr;
    if (hipHostMalloc(&h, kRingCap, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess || hipHostGetDevicePointer(&d, h, 0) != hipSuccess)
    {
      if (h) (void)hipHostFree(h);
      (void)hipGetLastError();
      c->ring_failed = true;
      return nullptr;
    }
    c->ring_host = (unsigned char *)h;
    c->ring_dev = (unsigned char *)d;
    c->ring_cap = kRingCap;
    c->ring_off = 0;
  }
  const size_t need = (bytes + 255u) & ~(size_t)255u;
  if (c->ring_off + need > c->ring_cap && stream_wait(c) != hipSuccess) return nullptr;
  unsigned char *h = c->ring_host + c->ring_off;
  *dev = c->ring_dev + c->ring_off;
  c->ring_off += need;
  return h;
}

// host -> device, `bytes` from pageable caller memory
static hipError_t copy_up(pllgpu_ctx *c, void *dst, const void *host, size_t bytes)
{
  unsigned char *dev = nullptr;
  if (unsigned char *h = stage_take(c, bytes, &dev))
  {
    memcpy(h, host, bytes);
    return hipMemcpyAsync(dst, h, bytes, hipMemcpyHostToDevice, c->stream);
  }
  return hipMemcpyAsync(dst, host, bytes, hipMemcpyHostToDevice, c->stream);
}

// Wait until a word of mapped host memory, stored by a kernel on the stream, carries `value`: a poll (a stream
// synchronise costs ~15 us of wake-up latency on a ~5 us kernel), and ONE stream synchronise once that has taken
// `limit_ms`, so that a failed launch cannot hang the caller - who checks the word again where it matters.
template <typename T>
static int wait_for_word(pllgpu_ctx *c, const T *word, T value, int limit_ms)
{
  const auto t0 = std::chrono::steady_clock::now();
  unsigned spins = 0;
  while (__atomic_load_n(word, __ATOMIC_ACQUIRE) != value)
    if ((++spins & 1023u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(limit_ms))
    {
      HIP_TRY(hipStreamSynchronize(c->stream));
      break;
    }
  return 0;
}

// wait until result[1] carries `sequence`, the word the last workgroup of a kernel stores next to its value
static int wait_for_sequence(pllgpu_ctx *c, double sequence)
{
  unsigned long long seq_bits;
  memcpy(&seq_bits, &sequence, sizeof seq_bits);
  return wait_for_word(c, (const unsigned long long *)&c->result_host[1], seq_bits, 20);
}

// device -> host and wait
static hipError_t copy_down(pllgpu_ctx *c, void *host, const void *src, size_t bytes)
{
  unsigned char *dev = nullptr;
  if (unsigned char *h = stage_take(c, bytes, &dev))
  {
    hipError_t e = hipMemcpyAsync(h, src, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e != hipSuccess) return e;
    c->pending_down.push_back({host, h, bytes});
    return c->defer_down ? hipSuccess : stream_wait(c);
  }
  const hipError_t e = hipMemcpyAsync(host, src, bytes, hipMemcpyDeviceToHost, c->stream);
  return e == hipSuccess ? stream_wait(c) : e;
}

extern "C" int pllgpu_download_defer(pllgpu_ctx_t *c, int on)
{
  CHECK_CTX_KEEP(c);
  c->defer_down = on != 0;
  if (!on && !c->pending_down.empty()) HIP_TRY(stream_wait(c));
  return 0;
}

extern "C" int pllgpu_clv_reserve(pllgpu_ctx_t *c, unsigned node, unsigned entries)
{
  CHECK_CTX(c);
  if (node >= c->geo.nodes) return fail(PLLGPU_EINVAL, "clv index %u out of range", node);
  return c->clv[node].ensure(clv_elems(c, entries));
}

extern "C" int pllgpu_clv_upload(pllgpu_ctx_t *c, unsigned node, const double *host, unsigned entries)
{
  CHECK_CTX(c); // (the context's device for the copies and the layout kernel below, not only for the reservation)
  if (int rc = pllgpu_clv_reserve(c, node, entries)) return rc;
  const size_t bytes = (size_t)entries * c->span * sizeof(double);
  c->clv_aos[node] = aos_entries(c, entries) ? 1 : 0;
  if (!c->tiled || c->clv_aos[node])
  {
    HIP_TRY(copy_up(c, c->clv[node].p, host, bytes));
    return 0;
  }
  unsigned char *dev = nullptr;
  if (unsigned char *h = stage_take(c, bytes, &dev))
  {
    // the layout kernel reads the caller's entries out of host memory
    memcpy(h, host, bytes);
    const unsigned blocks = (unsigned)std::min<size_t>(1024, ((size_t)(entries + 63u) * c->span + 255u) / 256u);
    hipLaunchKernelGGL(k_host_aos_to_tiled, dim3(blocks), dim3(256), 0, c->stream, reinterpret_cast<const double *>(dev), c->clv[node].p, entries,
                       c->gg.S, c->gg.SP, c->gg.R);
    HIP_TRY(hipGetLastError());
    return 0;
  }
  if (int rc = c->scratch.ensure((size_t)entries * c->span)) return rc;
  HIP_TRY(hipMemcpyAsync(c->scratch.p, host, bytes, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_aos_to_tiled, dim3(1024), dim3(256), 0, c->stream, c->scratch.p, c->clv[node].p, entries,
                     c->gg.S, c->gg.SP, c->gg.R);
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int pllgpu_clv_download(pllgpu_ctx_t *c, unsigned node, double *host, unsigned entries)
{
  CHECK_CTX(c);
  if (node >= c->geo.nodes || clv_elems(c, entries) > c->clv[node].cap)
    return fail(PLLGPU_EINVAL, "clv %u: download of %u entries exceeds the device buffer", node, entries);
  const size_t bytes = (size_t)entries * c->span * sizeof(double);
  const double *src = c->clv[node].p;
  if (c->tiled && !c->clv_aos[node])
  {
    unsigned char *dev = nullptr;
    if (unsigned char *h = stage_take(c, bytes, &dev))
    {
      // the layout kernel writes the entries into host memory
      const unsigned blocks = (unsigned)std::min<size_t>(1024, ((size_t)entries * c->span + 255u) / 256u);
      hipLaunchKernelGGL(k_host_tiled_to_aos, dim3(blocks), dim3(256), 0, c->stream, c->clv[node].p, reinterpret_cast<double *>(dev), entries,
                         c->gg.S, c->gg.SP, c->gg.R);
      HIP_TRY(hipGetLastError());
      c->pending_down.push_back({host, h, bytes});
      if (!c->defer_down) HIP_TRY(stream_wait(c));
      return 0;
    }
    if (int rc = c->scratch.ensure((size_t)entries * c->span)) return rc;
    hipLaunchKernelGGL(k_tiled_to_aos, dim3(1024), dim3(256), 0, c->stream, c->clv[node].p, c->scratch.p, entries,
                       c->gg.S, c->gg.SP, c->gg.R);
    HIP_TRY(hipGetLastError());
    src = c->scratch.p;
  }
  HIP_TRY(copy_down(c, host, src, bytes));
  return 0;
}

static inline size_t scaler_elems(const pllgpu_ctx *c, unsigned entries)
{
  return (size_t)entries * (c->geo.per_rate_scalers ? c->geo.rate_cats : 1u);
}

extern "C" int pllgpu_scaler_reserve(pllgpu_ctx_t *c, unsigned index, unsigned entries)
{
  CHECK_CTX(c);
  if (index >= c->geo.scale_buffers) return fail(PLLGPU_EINVAL, "scale buffer %u out of range", index);
  return c->scaler[index].ensure(scaler_elems(c, entries));
}

extern "C" int pllgpu_scaler_upload(pllgpu_ctx_t *c, unsigned index, const unsigned *host, unsigned entries)
{
  CHECK_CTX(c);
  if (int rc = pllgpu_scaler_reserve(c, index, entries)) return rc;
  HIP_TRY(copy_up(c, c->scaler[index].p, host, scaler_elems(c, entries) * sizeof(unsigned)));
  return 0;
}

extern "C" int pllgpu_scaler_download(pllgpu_ctx_t *c, unsigned index, unsigned *host, unsigned entries)
{
  CHECK_CTX(c);
  if (index >= c->geo.scale_buffers || scaler_elems(c, entries) > c->scaler[index].cap)
    return fail(PLLGPU_EINVAL, "scale buffer %u: download exceeds the device buffer", index);
  HIP_TRY(copy_down(c, host, c->scaler[index].p, scaler_elems(c, entries) * sizeof(unsigned)));
  return 0;
}

extern "C" int pllgpu_tipchars_upload(pllgpu_ctx_t *c, unsigned tip, const unsigned char *host, unsigned count)
{
  CHECK_CTX(c);
  if (tip >= c->geo.tips) return fail(PLLGPU_EINVAL, "tip %u out of range", tip);
  if (int rc = c->tipchars[tip].ensure(((size_t)count + 65) & ~(size_t)63)) return rc; // kernels fetch two codes at a time
  HIP_TRY(hipMemcpyAsync(c->tipchars[tip].p, host, count, hipMemcpyHostToDevice, c->stream));
  ++c->tips_epoch;
  return 0;
}

extern "C" int pllgpu_tipmap_upload(pllgpu_ctx_t *c, const unsigned long long *host, unsigned count)
{
  CHECK_CTX(c);
  if (!host)
  {
    c->tipmap_set = false;
    return 0;
  }
  if (int rc = c->tipmap.ensure(256)) return rc;
  HIP_TRY(hipMemcpyAsync(c->tipmap.p, host, std::min(count, 256u) * sizeof(unsigned long long),
                         hipMemcpyHostToDevice, c->stream));
  c->tipmap_set = true;
  c->tip_ncodes = 0;
  for (unsigned i = 0; i < std::min(count, 256u); ++i)
    if (host[i]) c->tip_ncodes = i + 1;
  ++c->maps_epoch; // cached launches carry the code count
  return 0;
}

// matrices [first, first+count) of the device block; slots prob_matrices and prob_matrices+1 hold the
// two sumtable contraction matrices (kernels_deriv.h)
static int upload_matrices(pllgpu_ctx *c, unsigned first, unsigned count, const double *host, unsigned limit)
{
  const pllgpu_geometry_t &g = c->geo;
  if (first + count > limit) return fail(PLLGPU_EINVAL, "matrix range [%u,%u) out of range", first, first + count);
  const unsigned S = g.states, SP = g.states_padded, R = g.rate_cats, SPT = c->gg.SPT;
  const size_t host_stride = (size_t)R * S * SP;
  // the device's layout is formed in pinned memory where the block fits (no wait), else in the staging vector
  const size_t doubles = c->pm_stride * count;
  unsigned char *dev = nullptr;
  double *stage = reinterpret_cast<double *>(stage_take(c, doubles * sizeof(double), &dev));
  if (stage)
    memset(stage, 0, doubles * sizeof(double));
  else
  {
    HIP_TRY(stream_wait(c)); // the previous async copy may still be reading the staging vector
    c->stage.assign(doubles, 0.0);
    stage = c->stage.data();
  }
  for (unsigned m = 0; m < count; ++m)
    for (unsigned k = 0; k < R; ++k)
      for (unsigned i = 0; i < S; ++i)
      {
        const double *row = host + m * host_stride + ((size_t)k * S + i) * SP;
        double *dst = stage + m * c->pm_stride + (size_t)k * S * SPT + i;
        for (unsigned j = 0; j < S; ++j) dst[(size_t)j * SPT] = row[j];
      }
  HIP_TRY(hipMemcpyAsync(c->pmat.p + (size_t)first * c->pm_stride, stage, doubles * sizeof(double), hipMemcpyHostToDevice, c->stream));
  for (unsigned m = first; m < first + count && m < c->pm_version.size(); ++m) ++c->pm_version[m];
  return 0;
}

extern "C" int pllgpu_pmatrix_upload(pllgpu_ctx_t *c, unsigned first, unsigned count, const double *host)
{
  // the matrix of the edge evaluated next is no input of the traversal before it and usually goes up between the two calls:
  // what is held stays held unless it reads one of these matrices
  CHECK_CTX_KEEP(c);
  if (int rc = matrices_change(c, nullptr, first, count)) return rc;
  return upload_matrices(c, first, count, host, c->geo.prob_matrices);
}

extern "C" int pllgpu_aux_matrix_upload(pllgpu_ctx_t *c, unsigned slot, const double *host)
{
  CHECK_CTX_KEEP_PENDING(c); // (no input of a CLV)
  if (slot > 1) return fail(PLLGPU_EINVAL, "aux matrix slot %u out of range", slot);
  return upload_matrices(c, c->geo.prob_matrices + slot, 1, host, c->geo.prob_matrices + 2);
}

extern "C" int pllgpu_frequencies_upload(pllgpu_ctx_t *c, unsigned index, const double *host)
{
  CHECK_CTX_KEEP_PENDING(c); // (no input of a CLV)
  if (index >= c->geo.rate_matrices) return fail(PLLGPU_EINVAL, "frequency set %u out of range", index);
  HIP_TRY(hipMemcpyAsync(c->freqs.p + (size_t)index * c->geo.states_padded, host,
                         c->geo.states_padded * sizeof(double), hipMemcpyHostToDevice, c->stream));
  return 0;
}

extern "C" int pllgpu_rate_weights_upload(pllgpu_ctx_t *c, const double *host)
{
  CHECK_CTX_KEEP_PENDING(c); // (no input of a CLV)
  HIP_TRY(hipMemcpyAsync(c->rate_weights.p, host, c->geo.rate_cats * sizeof(double), hipMemcpyHostToDevice, c->stream));
  return 0;
}

extern "C" int pllgpu_prop_invar_upload(pllgpu_ctx_t *c, const double *host)
{
  CHECK_CTX_KEEP_PENDING(c); // (no input of a CLV)
  HIP_TRY(hipMemcpyAsync(c->prop_invar.p, host, c->geo.rate_matrices * sizeof(double), hipMemcpyHostToDevice, c->stream));
  return 0;
}

extern "C" int pllgpu_pattern_weights_upload(pllgpu_ctx_t *c, const unsigned *host, unsigned count)
{
  CHECK_CTX_KEEP_PENDING(c); // (no input of a CLV)
  if (count > c->geo.sites_alloc) return fail(PLLGPU_EINVAL, "pattern weight count %u > %u", count, c->geo.sites_alloc);
  HIP_TRY(hipMemcpyAsync(c->pattern_weights.p, host, count * sizeof(unsigned), hipMemcpyHostToDevice, c->stream));
  if (c->rell) c->rell->stale = true; // (kernels_rell.h: the prefix sums are formed again before the next draw)
  return 0;
}

extern "C" int pllgpu_invariant_upload(pllgpu_ctx_t *c, const int *host, unsigned count)
{
  CHECK_CTX_KEEP_PENDING(c); // (no input of a CLV)
  if (!host)
  {
    c->invariant_set = false;
    return 0;
  }
  if (int rc = c->invariant.ensure(count)) return rc;
  HIP_TRY(hipMemcpyAsync(c->invariant.p, host, count * sizeof(int), hipMemcpyHostToDevice, c->stream));
  c->invariant_set = true;
  return 0;
}

// entries of a site -> class map buffer: whole groups of sixteen (kernels_repeats.h reads and writes them so)
static inline size_t map_elems(const pllgpu_ctx *c) { return ((size_t)c->geo.sites_alloc + 15u) / 16u * 16u; }

extern "C" int pllgpu_repeats_upload(pllgpu_ctx_t *c, unsigned node, const unsigned *site_id,
                                     const unsigned *id_site, unsigned ids)
{
  CHECK_CTX(c);
  if (node >= c->geo.nodes) return fail(PLLGPU_EINVAL, "node %u out of range", node);
  c->ids[node] = ids;
  ++c->maps_epoch;
  ++c->maps_version;
  ++c->maps_foreign;
  c->map_widened[node] = 0;
  c->rep_left[node] = c->rep_right[node] = -1; // host-built maps: no entry-indexed child maps
  c->map_forms[node] = 0;
  if (!ids) return 0;
  if (int rc = c->id_site[node].ensure(ids)) return rc;
  if (id_site) HIP_TRY(copy_up(c, c->id_site[node].p, id_site, ids * sizeof(unsigned)));
  if (ids <= kRepNarrow)
  {
    // at most 256 classes - every tip: the map goes up as BYTES (a quarter of the bus: 128 tips x 1M sites were 512 MB), the
    // form the class kernels read; the 32-bit form the site-indexed gathers and the API want is made on the device on demand
    if (int rc = c->site_id8[node].ensure(map_elems(c))) return rc;
    c->stage8.resize(c->geo.sites_alloc);
    for (unsigned s = 0; s < c->geo.sites_alloc; ++s) c->stage8[s] = (unsigned char)site_id[s];
    HIP_TRY(hipMemcpyAsync(c->site_id8[node].p, c->stage8.data(), c->geo.sites_alloc, hipMemcpyHostToDevice, c->stream)); // (pageable: staged before it returns)
    c->map_forms[node] = kMap8;
    return 0;
  }
  if (int rc = c->site_id[node].ensure(map_elems(c))) return rc;
  HIP_TRY(hipMemcpyAsync(c->site_id[node].p, site_id, c->geo.sites_alloc * sizeof(unsigned), hipMemcpyHostToDevice, c->stream));
  c->map_forms[node] = kMap32;
  return 0;
}

// The 32-bit form of a node's site -> class map, produced from the byte form if that is what the class kernels left
// (kernels_repeats.h); nullptr if the node has no maps on the device. Callers: the gathering launches that index by site,
// the edge / root / derivative evaluations, the copy to the host.
static const unsigned *wide_map(pllgpu_ctx *c, unsigned node)
{
  if (c->map_forms[node] & kMap32) return c->site_id[node].p;
  if (!(c->map_forms[node] & kMap8)) return c->site_id[node].p; // (uploaded by an older path or never written: as before)
  if (c->site_id[node].ensure(map_elems(c))) return nullptr;
  const unsigned n = (unsigned)map_elems(c);
  hipLaunchKernelGGL(k_rep_widen, dim3((n / 16u + 255u) / 256u), dim3(256), 0, c->stream, c->site_id8[node].p, c->site_id[node].p, n);
  c->map_forms[node] |= kMap32;
  c->map_widened[node] = 1; // from now on the class kernels' bytes are followed by this form again (pllgpu_repeats_classes)
  return c->site_id[node].p;
}

static int narrow_map(pllgpu_ctx *c, unsigned node)
{
  if (c->map_forms[node] & kMap8) return 0;
  if (!(c->map_forms[node] & kMap32) || !c->site_id[node].p) return fail(PLLGPU_EINVAL, "node %u has no class maps on the device", node);
  if (int rc = c->site_id8[node].ensure(map_elems(c))) return rc;
  const unsigned n = (unsigned)map_elems(c);
  hipLaunchKernelGGL(k_rep_narrow, dim3((n / 16u + 255u) / 256u), dim3(256), 0, c->stream, c->site_id[node].p, c->site_id8[node].p, n);
  c->map_forms[node] |= kMap8;
  return 0;
}

// ---- launches --------------------------------------------------------------------------------
// Run-time values that select a template instantiation: each helper hands its generic lambda the values as
// std::integral_constant arguments (LT() etc. are constant expressions there) - for exactly the combinations
// that have a kernel, no others are instantiated.
template <bool B>
using Bool = std::integral_constant<bool, B>;
template <int I>
using Int = std::integral_constant<int, I>;

// two flags, e.g. (the child end of an edge is a tip, gather) -> fn(CT, GA)
template <class F>
static void with_bools(bool a, bool b, F &&fn)
{
  if (a)
  {
    if (b) fn(Bool<true>(), Bool<true>()); else fn(Bool<true>(), Bool<false>());
  }
  else
  {
    if (b) fn(Bool<false>(), Bool<true>()); else fn(Bool<false>(), Bool<false>());
  }
}

// the children of a level launch, kind = number of tip children (a tip-inner op carries its tip on the left) -> fn(LT, RT)
template <class F>
static void with_child_tips(unsigned kind, F &&fn)
{
  if (kind == 0) fn(Bool<false>(), Bool<false>());
  else if (kind == 1) fn(Bool<true>(), Bool<false>());
  else fn(Bool<true>(), Bool<true>());
}

// ... and whether the launch gathers -> fn(LT, RT, GA)
template <class F>
static void with_children(unsigned kind, bool gather, F &&fn)
{
  with_child_tips(kind, [&](auto LT, auto RT) {
    if (gather) fn(LT, RT, Bool<true>()); else fn(LT, RT, Bool<false>());
  });
}

// an index below N -> fn(Int<i>)
template <class F, int... I>
static void with_index(unsigned i, F &&fn, std::integer_sequence<int, I...>)
{
  ((i == (unsigned)I ? (void)fn(Int<I>()) : (void)0), ...);
}

// the accumulator chunk of the FMA kernels (c->ich: 4, 8, 16, 20, anything else runs as 32) -> fn(Int<ICH>)
template <class F>
static void with_ich(int ich, F &&fn)
{
  switch (ich)
  {
    case 4: fn(Int<4>()); break;
    case 8: fn(Int<8>()); break;
    case 16: fn(Int<16>()); break;
    case 20: fn(Int<20>()); break;
    default: fn(Int<32>()); break;
  }
}

// the chain kernels (kernels_dna.h): the scaling mode and which fetch groups a chain's steps issue (ChainLaunchRec::variant)
// -> fn(SMV, C0, S1, C1). One table for the chain launches and for the edge kernels that take held chains over: they
// must agree on it.
template <class F>
static void with_chain_variant(int scale_mode, unsigned variant, F &&fn)
{
  auto fetches = [&](auto SMV) {
    switch (variant)
    {
      case 0: fn(SMV, Bool<false>(), Bool<false>(), Bool<false>()); break;
      case 1: fn(SMV, Bool<false>(), Bool<true>(), Bool<false>()); break;
      case 2: fn(SMV, Bool<true>(), Bool<false>(), Bool<false>()); break;
      default: fn(SMV, Bool<true>(), Bool<true>(), Bool<true>()); break;
    }
  };
  if (scale_mode == 2) fetches(Int<2>()); else fetches(Int<1>());
}

// a pair of DnaChildKind out of the listed ones -> fn(A, B) and true; false for a pair that is not listed (no kernel)
template <int A, int B>
struct KindPair
{
};
template <class F, int... A, int... B>
static bool with_kind_pair(int a, int b, F &&fn, KindPair<A, B>...)
{
  return ((a == A && b == B ? (fn(Int<A>(), Int<B>()), true) : false) || ...);
}

// what the launches issued so far have left behind
static int launch_status()
{
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(PLLGPU_ERUNTIME, "kernel launch failed: %s", hipGetErrorString(e));
  return 0;
}

static const unsigned long long *tipmap_ptr(const pllgpu_ctx *c) { return c->tipmap_set ? c->tipmap.p : nullptr; }
static int resolve_op(pllgpu_ctx *c, const pllgpu_op_t &o, DevOp &d)
{
  const pllgpu_geometry_t &g = c->geo;
  if (o.parent_clv >= g.nodes || o.left_clv >= g.nodes || o.right_clv >= g.nodes)
    return fail(PLLGPU_EINVAL, "operation references a CLV out of range");
  if (o.left_matrix >= g.prob_matrices || o.right_matrix >= g.prob_matrices)
    return fail(PLLGPU_EINVAL, "operation references a p-matrix out of range");
  memset(&d, 0, sizeof d);
  if (int rc = c->clv[o.parent_clv].ensure(clv_elems(c, o.parent_entries))) return rc;
  d.parent = c->clv[o.parent_clv].p;
  d.entries = o.parent_entries;
  // layout of the three CLVs (4x4 only): what the children were written as, what the parent becomes
  c->clv_aos[o.parent_clv] = aos_entries(c, o.parent_entries) ? 1 : 0;
  if (c->clv_aos[o.parent_clv]) c->any_aos = true;
  d.layout = c->clv_aos[o.parent_clv] ? kAosParent : 0u;
  if (!(o.flags & PLLGPU_OP_LEFT_TIP) && c->clv_aos[o.left_clv]) d.layout |= kAosLeft;
  if (!(o.flags & PLLGPU_OP_RIGHT_TIP) && c->clv_aos[o.right_clv]) d.layout |= kAosRight;
  if (d.layout && !(o.flags & PLLGPU_OP_GATHER)) return fail(PLLGPU_EINVAL, "a class-compressed CLV met an operation without the gather flag");
  // a compressed child with about as many entries as the parent is read once per entry: streaming loads;
  // a much smaller one is a table the parent's tiles keep coming back to: cacheable loads
  if ((d.layout & kAosLeft) && (size_t)c->ids[o.left_clv] * 2u > o.parent_entries) d.layout |= kStreamLeft;
  if ((d.layout & kAosRight) && (size_t)c->ids[o.right_clv] * 2u > o.parent_entries) d.layout |= kStreamRight;
  if (o.flags & PLLGPU_OP_LEFT_TIP)
  {
    if (o.left_clv >= g.tips || !c->tipchars[o.left_clv].p) return fail(PLLGPU_EINVAL, "tip %u has no codes on the device", o.left_clv);
    d.ltip = c->tipchars[o.left_clv].p;
  }
  else
  {
    if (!c->clv[o.left_clv].p) return fail(PLLGPU_EINVAL, "CLV %u was never computed or uploaded", o.left_clv);
    d.left = c->clv[o.left_clv].p;
  }
  if (o.flags & PLLGPU_OP_RIGHT_TIP)
  {
    if (o.right_clv >= g.tips || !c->tipchars[o.right_clv].p) return fail(PLLGPU_EINVAL, "tip %u has no codes on the device", o.right_clv);
    d.rtip = c->tipchars[o.right_clv].p;
  }
  else
  {
    if (!c->clv[o.right_clv].p) return fail(PLLGPU_EINVAL, "CLV %u was never computed or uploaded", o.right_clv);
    d.right = c->clv[o.right_clv].p;
  }
  auto scal = [&](int idx, const unsigned *&out, unsigned need) -> int {
    out = nullptr;
    if (idx < 0) return 0;
    if ((unsigned)idx >= g.scale_buffers) return fail(PLLGPU_EINVAL, "scale buffer %d out of range", idx);
    if (need)
    {
      if (int rc = c->scaler[idx].ensure(scaler_elems(c, need))) return rc;
    }
    else if (!c->scaler[idx].p)
      return fail(PLLGPU_EINVAL, "scale buffer %d read before it was written", idx);
    out = c->scaler[idx].p;
    return 0;
  };
  const unsigned *ps = nullptr;
  if (int rc = scal(o.parent_scaler, ps, o.parent_entries)) return rc;
  d.pscaler = const_cast<unsigned *>(ps);
  if (int rc = scal(o.left_scaler, d.lscaler, 0)) return rc;
  if (int rc = scal(o.right_scaler, d.rscaler, 0)) return rc;
  d.lmat = c->pmat.p + (size_t)o.left_matrix * c->pm_stride;
  d.rmat = c->pmat.p + (size_t)o.right_matrix * c->pm_stride;
  if (o.flags & PLLGPU_OP_GATHER)
  {
    const unsigned p = o.parent_clv;
    if (c->ids[p] && c->rep_left[p] == (int)o.left_clv && c->rep_right[p] == (int)o.right_clv)
    {
      d.lsid = c->lent[p].p; // entry-indexed: two coalesced loads per lane
      d.rsid = c->rent[p].p;
      d.layout |= kDirectMaps;
    }
    else if (c->ids[p] && c->rep_left[p] == (int)o.right_clv && c->rep_right[p] == (int)o.left_clv)
    {
      d.lsid = c->rent[p].p; // the host put the tip on the left
      d.rsid = c->lent[p].p;
      d.layout |= kDirectMaps;
    }
    else
    {
      d.id_site = c->ids[p] ? c->id_site[p].p : nullptr;
      d.lsid = c->ids[o.left_clv] ? wide_map(c, o.left_clv) : nullptr;
      d.rsid = c->ids[o.right_clv] ? wide_map(c, o.right_clv) : nullptr;
      if ((c->ids[o.left_clv] && !d.lsid) || (c->ids[o.right_clv] && !d.rsid)) return fail(PLLGPU_EINVAL, "operation gathers through class maps that are not on the device");
    }
  }
  return 0;
}

// the workgroup of every kernel over the tiled layout: one wave per rate category of the tile, up to 4
static unsigned tiled_waves(const pllgpu_ctx *c) { return std::min(c->gg.R, 4u); }
static unsigned tiled_threads(const pllgpu_ctx *c) { return 64u * tiled_waves(c); }

template <int ICH>
static void launch_generic(pllgpu_ctx *c, const OpPack &pack, unsigned nops, unsigned maxent, unsigned kind, bool gather)
{
  // one workgroup per 64-entry tile; min(R,4) waves share the tile's rate categories
  const unsigned tiles = (maxent + 63) / 64;
  const unsigned long long *tm = tipmap_ptr(c);
  // tip children: room in LDS for the staged matrices of every wave (kernels_generic.h: tip_stage)
  const unsigned nw = tiled_waves(c);
  const bool stage = kind != 0 && c->gg.S * c->gg.SPT <= 1024u && !c->no_tip_columns;
  const unsigned tip_lds = stage ? 1u : 0u;
  size_t lds = stage ? (size_t)2 * nw * (c->gg.S + 1u) * (c->gg.SPT | 1u) * sizeof(double) : 0;
  // entry-contiguous parents leave through LDS (kernels_generic.h): 16-byte rows need states_padded % 4 == 0
  // and entry-contiguous children arrive through it, SP / 2 lanes per (entry, rate)
  bool any_aos = false;
  for (unsigned i = 0; i < nops; ++i) any_aos = any_aos || (pack.ops[i].layout & (kAosParent | kAosLeft | kAosRight));
  const unsigned par_lds = (gather && any_aos && c->gg.SP % 4u == 0 && (ICH != 20 || c->gg.SP == 20u) && !c->no_par_lds) ? (c->no_coop_fetch ? 2u : 1u) : 0u;
  if (par_lds) lds += (size_t)nw * 64u * (c->gg.SP + 2u) * sizeof(double);

  // staged tip matrices are shared by the tiles of a workgroup: several tiles each, as long as
  // ~2048 workgroups remain
  unsigned tpb = 1;
  // (staging costs a workgroup about as much as four tiles of work: C3's 32-op launch 259 us with up to 8
  // tiles per workgroup and >= 4096 workgroups, 247 us with up to 16 and >= 2048, 268 us with 32 / 1024)
  if (stage) tpb = std::max(1u, std::min(16u, (unsigned)(((size_t)tiles * nops) / 2048u)));
  dim3 grid((tiles + tpb - 1) / tpb, nops), block(64u * nw);
  // the kernel and, for the same instantiation, its LDS limit
  auto launch = [&](auto LT, auto RT, auto GA, auto LAY) {
    const auto kernel = k_partials_tiled<ICH, LT(), RT(), GA(), LAY()>;
    if (par_lds) raise_lds_limit((const void *)kernel, c->device, lds);
    hipLaunchKernelGGL(kernel, grid, block, lds, c->stream, pack, c->gg, tm, tip_lds, tpb, par_lds);
  };
  if constexpr (ICH == 20)
    if (gather)
    {
      // the protein shape: when every op of the launch has the same CLV layouts (the rule: a level of a tree), the
      // instantiation that knows them at compile time
      const unsigned lay = pack.ops[0].layout & 7u;
      bool same = true;
      for (unsigned i = 1; i < nops; ++i) same = same && (pack.ops[i].layout & 7u) == lay;
      if (same)
      {
        with_child_tips(kind, [&](auto LT, auto RT) {
          with_index(lay, [&](auto LAY) { launch(LT, RT, Bool<true>(), LAY); }, std::make_integer_sequence<int, 8>());
        });
        return;
      }
    }
  with_children(kind, gather, [&](auto LT, auto RT, auto GA) { launch(LT, RT, GA, Int<-1>()); });
}

static void launch_dna(pllgpu_ctx *c, const OpPack &pack, unsigned nops, unsigned maxent, unsigned kind, bool gather)
{
  // one wave per 64-site tile (kDnaTilesPerWave, kernels_dna.h)
  const unsigned tiles = (maxent + 63) / 64;
  const unsigned tpw = kDnaTilesPerWave;
  const unsigned nx = (tiles + 4 * tpw - 1) / (4 * tpw);
  dim3 grid = xcd_grid(nx, nops), block(256);
  const int mode = c->gg.scale_mode;
  // gathering launches: a pattern-sorted alignment's neighbouring sites gather neighbouring entries, and with the XCD-aware
  // order (kernels_common.h) an XCD's L2 holds the entries of ITS run of sites, not a copy of everybody's
  const unsigned xcd = (c->xcd_order && gather) ? 1u : 0u;
  with_children(kind, gather, [&](auto LT, auto RT, auto GA) {
    hipLaunchKernelGGL((k_partials_dna<LT(), RT(), GA()>), grid, block, 0, c->stream, pack, mode, tpw, nx, nops, xcd);
  });
}

// site repeats: (gathering, gathering -> inner x inner) groups (kernels_dna.h: k_partials_dna_gg)
static void launch_gg(pllgpu_ctx *c, const GGPack &pack, unsigned ngroups, unsigned entries)
{
  const unsigned tiles = (entries + 63) / 64;
  const unsigned tpw = kDnaTilesPerWave;
  const unsigned nx = (tiles + 4 * tpw - 1) / (4 * tpw);
  dim3 grid = xcd_grid(nx, ngroups), block(256);
  const unsigned stream_parent = ((size_t)ngroups * entries * 128u > c->stream_parent_bytes) ? 1u : 0u;
  const unsigned xcd = c->xcd_order; // (C4's shard, same box: 0.1104-0.1111 -> 0.1089-0.1102 ms per step for the slowest shards)
  hipLaunchKernelGGL(k_partials_dna_gg, grid, block, 0, c->stream, pack, entries, c->gg.scale_mode, tpw, stream_parent, nx, ngroups, xcd);
}

// fp64 MFMA 4x4x4 kernels, matrices staged in LDS (kernels_mfma.h): NG = number of 4-state groups
// k_partials_mfma_wide counts its own vector-memory operations (kernels_mfma_wide.h): a register spilled to scratch
// would be one the count does not know about. The build is checked once per process; a compiler that spills sends the
// shape back to the first-generation kernel (and says so). This run-time look sees scratch only; what a compiler could
// also do - copy, move or park in accumulation registers a load's destination before its wait - is checked where it
// can be seen, on the emitted instructions at build time (tools/check_wide_isa.py, a prerequisite of libpll_amd.so in
// the Makefile; tests/test_wide_isa_check.py plants those failures into the real instruction stream).
template <int NGJ, int TAIL, int WAVES>
static bool wide_kernel_is_sound()
{
  static int st = -1;
  if (st < 0)
  {
    hipFuncAttributes at;
    st = (hipFuncGetAttributes(&at, (const void *)k_partials_mfma_wide<NGJ, TAIL, WAVES>) == hipSuccess && at.localSizeBytes == 0) ? 1 : 0;
    if (!st) fprintf(stderr, "libpll_amd: k_partials_mfma_wide was built with scratch memory; using k_partials_mfma instead\n");
  }
  return st == 1;
}

// One round of workgroups, one (8 waves) or two (4 waves) per CU; every (op, rate category) gets the same number of
// them and cuts its half tiles into that many runs.
template <int NGJ, int TAIL, int WAVES>
static bool launch_wide(pllgpu_ctx *c, const OpPack &pack, unsigned nops, unsigned halves, unsigned char *fb, unsigned fstride)
{
  if (!wide_kernel_is_sound<NGJ, TAIL, WAVES>()) return false;
  const unsigned R = c->gg.R, max_wgs = 2048u / WAVES;
  const unsigned per_pair = std::max(1u, max_wgs / (nops * R));
  const unsigned hw = std::max(1u, (halves + per_pair - 1) / per_pair);
  dim3 grid((halves + hw - 1) / hw, nops, R), block(64 * WAVES);
  const size_t lds = MfmaGeo<16>::lds_doubles * sizeof(double);
  raise_lds_limit((const void *)k_partials_mfma_wide<NGJ, TAIL, WAVES>, c->device, lds);
  hipLaunchKernelGGL((k_partials_mfma_wide<NGJ, TAIL, WAVES>), grid, block, lds, c->stream, pack, c->gg, hw, fb, fstride);
  return true;
}


// Does a matrix-pipe launch rescale, and where do its kernels leave the flag bytes that k_mfma_scale_epilogue reads.
// min_bytes: k_partials_mfma_wide forms a buffer descriptor over the block even when nothing is rescaled (size 0, every
// lane dropped: kernels_mfma_wide.h), so its launch is given 64 real bytes to point at; the other kernels do not look at
// the pointer then and reserve nothing.
struct MfmaScaling
{
  bool scaling = false;
  unsigned fstride = 0;
  unsigned char *flags = nullptr;
};

static int mfma_scaling(pllgpu_ctx *c, bool any_parent_scaler, unsigned entries, size_t min_bytes, MfmaScaling &s)
{
  s.scaling = any_parent_scaler && c->gg.scale_mode != 0;
  s.fstride = (entries + 63u) & ~63u;
  if (c->mfma_flags.ensure(std::max(min_bytes, s.scaling ? (size_t)kMaxOpsPerLaunch * c->gg.R * s.fstride : (size_t)0))) return PLLGPU_ENOMEM;
  s.flags = c->mfma_flags.p;
  return 0;
}

static int mfma_scaling(pllgpu_ctx *c, const OpPack &pack, unsigned nops, unsigned entries, size_t min_bytes, MfmaScaling &s)
{
  bool any = false;
  for (unsigned i = 0; i < nops; ++i) any = any || pack.ops[i].pscaler != nullptr;
  return mfma_scaling(c, any, entries, min_bytes, s);
}

// the parents' scalers from the flag bytes; gather: the parents' entries are found through their class maps
static void launch_scale_epilogue(pllgpu_ctx *c, const OpPack &pack, unsigned nops, unsigned entries, const MfmaScaling &s, bool gather)
{
  if (!s.scaling) return;
  dim3 eg((entries + 255) / 256, nops);
  if (gather)
    hipLaunchKernelGGL((k_mfma_scale_epilogue<true>), eg, dim3(256), 0, c->stream, pack, c->gg, s.flags, s.fstride);
  else
    hipLaunchKernelGGL((k_mfma_scale_epilogue<false>), eg, dim3(256), 0, c->stream, pack, c->gg, s.flags, s.fstride);
}

template <int NG>
static int launch_mfma_t(pllgpu_ctx *c, const OpPack &pack, unsigned nops, unsigned maxent, unsigned kind, bool gather)
{
  const unsigned R = c->gg.R;
  const unsigned items = (maxent + 31) / 32; // 32 sites per item
  MfmaScaling s;
  if (NG == 16 && kind == 0 && !gather && c->mfma_wide)
  {
    // 33..64 states, inner x inner, tiled CLVs: the second-generation kernel (kernels_mfma_wide.h). Work is dealt in
    // half tiles: every SIMD gets two waves and the pair the same number of half tiles, give or take one
    if (int rc = mfma_scaling(c, pack, nops, maxent, 64, s)) return rc;
    const bool exact61 = c->gg.S == 61 && !c->mfma_pad;
    // (8-wave workgroups, one per CU: against two of 4 waves the matrices are staged once per CU and a SIMD's two waves
    // split an odd share - C5's 2-op launch 66 -> 58 us, the step 0.549 -> 0.537 ms, profiles/README.md round 3)
    const bool done = exact61 ? launch_wide<15, 1, 8>(c, pack, nops, items, s.flags, s.fstride) : launch_wide<16, 0, 8>(c, pack, nops, items, s.flags, s.fstride);
    if (done)
    {
      launch_scale_epilogue(c, pack, nops, maxent, s, false);
      return 0;
    }
  }
  if (int rc = mfma_scaling(c, pack, nops, maxent, 0, s)) return rc;
  if (kind == 2 && !gather && NG > 8 && c->tt_stream && !c->no_tip_columns)
  {
    // plain tip x tip level of a large state space: a store stream, lane = site (kernels_mfma.h: k_partials_tt_stream)
    const unsigned tiles = (maxent + 63u) / 64u;
    constexpr unsigned nw = kTtStreamThreads / 64u; // waves of a workgroup
    // workgroups: each stages its rate category's two matrices (2 x 30 KB for 61 states) first, two fit a CU - one round of
    // them (C5, same box: 1 / 2 / 3 / 5 tiles per wave = 1280 / 640 / 448 / 256 workgroups: 101.6 / 106.5 / 99.8 / 98.8 us)
    const unsigned want = 512u;
    unsigned tpw = (unsigned)(((size_t)((tiles + nw - 1u) / nw) * nops * R + want - 1u) / want);
    tpw = std::max(1u, tpw);
    const unsigned nx = (tiles + nw * tpw - 1u) / (nw * tpw);
    const unsigned S = c->gg.S;
    const size_t lds = 2u * (size_t)(S + 1u) * tt_stream_ld(S) * sizeof(double);
    raise_lds_limit((const void *)k_partials_tt_stream, c->device, lds);
    hipLaunchKernelGGL(k_partials_tt_stream, xcd_grid(nx, nops, R), dim3(kTtStreamThreads), lds, c->stream, pack, c->gg, tipmap_ptr(c), tpw, s.flags, s.fstride, nx, nops, c->xcd_order);
    launch_scale_epilogue(c, pack, nops, maxent, s, false);
    return 0;
  }
  // aim at two workgroups of four waves on every CU (2048 waves) - four where the small shapes leave room;
  // more work -> more items per wave. (Round 4, C5's tip x tip launch with 1024 / 2048 / 4096 / 8192 / 16384 / 40000
  // waves wanted: 1020 / 1063 / 1076 / 1051 / 1020 / 908 M updates/s for the step - flat around the choice, unlike the
  // 4 x 4 kernels, which gained 6 % from one tile per wave: every workgroup here stages 64 KB of matrices first)
  const unsigned want = NG > 8 ? 2048u : 4096u;
  unsigned ipw = (unsigned)(((size_t)items * nops * R + want - 1) / want);
  ipw = std::max(1u, std::min(ipw, NG > 8 ? ~0u : 8u));
  dim3 grid((items + 4 * ipw - 1) / (4 * ipw), nops, R), block(256);
  // (round 5 ran the plain tip x tip levels - store traffic and nothing else, C5's: 625 MB - in the XCD-aware order of the
  // other store-bound launches as well: 119.7 -> 122.7 us, profiles/README.md; the switch and its code are gone)
  const size_t lds = MfmaGeo<NG>::lds_doubles * sizeof(double);
  const unsigned long long *tm = tipmap_ptr(c);
  with_children(kind, gather, [&](auto LT, auto RT, auto GA) {
    const auto kernel = k_partials_mfma<NG, LT(), RT(), GA()>;
    raise_lds_limit((const void *)kernel, c->device, lds);
    hipLaunchKernelGGL(kernel, grid, block, lds, c->stream, pack, c->gg, tm, ipw, s.flags, s.fstride);
  });
  launch_scale_epilogue(c, pack, nops, maxent, s, gather);
  return 0;
}

// (tip x tip, tip x tip -> inner x inner) groups on the matrix pipe (kernels_mfma.h: k_partials_mfma_cc)
template <int NG>
static int launch_mfma_cc_t(pllgpu_ctx *c, const FusePack &pack, unsigned ngroups, unsigned entries)
{
  const unsigned R = c->gg.R, S = c->gg.S;
  const unsigned items = (entries + 31) / 32;
  // store-bound: many small workgroups - but each stages its six matrices and two tables (20-50 KB from L2), so not
  // too small: C3 (1563 items x 16 groups x 4 rates) with 8 / 4 / 2 / 1 items per wave and the XCD-aware order: step
  // 0.550 / 0.537 / 0.563 / 0.622 ms on one box (round 4, tools/round4_calls/r4_c3_exp.sh; natural order: 0.555 / - / 0.622 / -);
  // 3 / 4 / 5 / 6 on another: 0.551-0.554 / 0.549-0.558 / 0.550-0.554 / 0.553-0.557 - flat between three and six
  const unsigned want = 4096u;
  unsigned ipw = (unsigned)(((size_t)items * ngroups * R + want - 1) / want);
  ipw = std::max(1u, std::min(ipw, 4u));
  const unsigned nx = (items + 4 * ipw - 1) / (4 * ipw);
  dim3 grid = xcd_grid(nx, ngroups, R), block(256);
  const unsigned long long *tm = tipmap_ptr(c);
  const unsigned ncodes = c->tip_ncodes;
  const size_t lds = CcGeo<NG>::lds_bytes(ncodes);
  // which cherries are rescaled: per pair of tip codes, every rate's answer (k_cherry_bits) - a table per pair of
  // tip matrices, kept on the device until one of the two is written again
  {
    const unsigned char *before = c->cherry_bits.p;
    if (int rc = c->cherry_bits.ensure((size_t)kCherrySlots * R * ncodes * ncodes)) return rc;
    if (c->cherry_bits.p != before || c->cherry_slot.size() != kCherrySlots)
    {
      c->cherry_slot_of.clear(); // a fresh block: no table survives
      c->cherry_slot.assign(kCherrySlots, pllgpu_ctx::CherrySlot());
    }
  }
  CherryTips stale;
  memset(&stale, 0, sizeof stale);
  unsigned nstale = 0;
  CherrySlots slots;
  memset(&slots, 0, sizeof slots);
  OpPack parents; // the group parents as plain ops: what the scaling epilogue works on
  memset(&parents, 0, sizeof parents);
  bool any_parent_scaler = false;
  if (c->cherry_slot_of.size() + 2 * ngroups > kCherrySlots)
  {
    // full: start over (launches already in the stream read their tables before any of them is overwritten)
    c->cherry_slot_of.clear();
    c->cherry_slot.assign(kCherrySlots, pllgpu_ctx::CherrySlot());
  }
  for (unsigned i = 0; i < ngroups; ++i)
  {
    for (unsigned ch = 0; ch < 2; ++ch)
    {
      const FOp &f = ch ? pack.g[i].b : pack.g[i].a;
      const unsigned long long li = (unsigned long long)((f.lmat - c->pmat.p) / (ptrdiff_t)c->pm_stride),
                               ri = (unsigned long long)((f.rmat - c->pmat.p) / (ptrdiff_t)c->pm_stride);
      auto ins = c->cherry_slot_of.emplace((li << 32) | ri, (unsigned)c->cherry_slot_of.size());
      const unsigned sl = ins.first->second;
      pllgpu_ctx::CherrySlot &cs = c->cherry_slot[sl];
      slots.s[2 * i + ch] = (unsigned short)sl;
      if (cs.lver != c->pm_version[li] || cs.rver != c->pm_version[ri] || cs.maps != c->maps_epoch + 1ull)
      {
        cs.lver = c->pm_version[li];
        cs.rver = c->pm_version[ri];
        cs.maps = c->maps_epoch + 1ull;
        bool listed = false; // the same pair of matrices twice in one launch: one table
        for (unsigned q = 0; q < nstale; ++q) listed = listed || stale.slot[q] == sl;
        if (!listed)
        {
          stale.lmat[nstale] = f.lmat;
          stale.rmat[nstale] = f.rmat;
          stale.slot[nstale] = (unsigned short)sl;
          ++nstale;
        }
      }
    }
    DevOp &d = parents.ops[i];
    d.parent = pack.g[i].p.parent;
    d.pscaler = pack.g[i].p.pscaler;
    d.lscaler = pack.g[i].a.pscaler;
    d.rscaler = pack.g[i].b.pscaler;
    d.entries = entries;
    any_parent_scaler = any_parent_scaler || d.pscaler != nullptr;
  }
  if (nstale)
  {
    size_t bits_lds = ((size_t)2 * S * S + (size_t)2 * ncodes * S) * sizeof(double);
    const unsigned staged = bits_lds <= 144u * 1024u ? 1u : 0u;
    if (!staged) bits_lds = (size_t)2 * ncodes * S * sizeof(double);
    raise_lds_limit((const void *)k_cherry_bits, c->device, bits_lds);
    hipLaunchKernelGGL(k_cherry_bits, dim3(nstale, R), dim3(256), bits_lds, c->stream, stale, c->gg, tm, ncodes, c->cherry_bits.p,
                       nullptr, staged);
  }
  MfmaScaling s;
  if (int rc = mfma_scaling(c, any_parent_scaler, entries, 0, s)) return rc;
  raise_lds_limit((const void *)k_partials_mfma_cc<NG>, c->device, lds);
  // parents beyond what the Infinity Cache keeps for the next level: streamed out like the cherries (as the 4x4 groups do)
  const unsigned stream_parent = ((size_t)ngroups * entries * S * R * 8u > c->stream_parent_bytes) ? 1u : 0u;
  hipLaunchKernelGGL((k_partials_mfma_cc<NG>), grid, block, lds, c->stream, pack, c->gg, tm, entries, ipw, s.flags, s.fstride,
                     c->cherry_bits.p, slots, ncodes, stream_parent, nx, ngroups, c->xcd_order);
  launch_scale_epilogue(c, parents, ngroups, entries, s, false);
  return 0;
}

static int launch_mfma_cc(pllgpu_ctx *c, const FusePack &pack, unsigned ngroups, unsigned entries)
{
  if (c->mfma_ng == 5) return launch_mfma_cc_t<5>(c, pack, ngroups, entries);
  return launch_mfma_cc_t<8>(c, pack, ngroups, entries);
}

static int launch_mfma(pllgpu_ctx *c, const OpPack &pack, unsigned nops, unsigned maxent, unsigned kind, bool gather)
{
  switch (c->mfma_ng)
  {
    case 5: return launch_mfma_t<5>(c, pack, nops, maxent, kind, gather);
    case 8: return launch_mfma_t<8>(c, pack, nops, maxent, kind, gather);
    default: return launch_mfma_t<16>(c, pack, nops, maxent, kind, gather);
  }
}

// 17..20 states, up to four rate categories: every level launch on the matrix pipe (kernels_lean.h)
static int launch_lean(pllgpu_ctx *c, const OpPack &pack, unsigned nops, unsigned maxent, unsigned kind, bool gather)
{
  const unsigned R = c->gg.R;
  const unsigned items = (maxent + 31) / 32;
  // staging the workgroup's matrices costs about as much as two items: several items per workgroup, as long as
  // a few thousand workgroups remain
  unsigned ipb = (unsigned)(((size_t)items * nops) / 4096u);
  ipb = std::max(2u, std::min(ipb, 16u));
  // a tip x tip item is two dozen LDS reads and five stores: staging has to be spread over more of them (C3's 32 cherries:
  // 295 / 240 / 205 / 204 / 254 us with 2 / 8 / 16 / 32 / 64 items per workgroup)
  if (kind == 2 && !gather) ipb = std::max(2u, std::min((unsigned)(((size_t)items * nops) / 1536u), 32u));
  dim3 grid((items + ipb - 1) / ipb, nops), block(64u * R);
  const size_t lds = LeanGeo<5>::lds_bytes(R, gather);
  const unsigned long long *tm = tipmap_ptr(c);
  const unsigned ncodes = std::min(c->tip_ncodes, 256u);
  with_children(kind, gather, [&](auto LT, auto RT, auto GA) {
    const auto kernel = k_partials_lean<5, LT(), RT(), GA()>;
    if (GA()) raise_lds_limit((const void *)kernel, c->device, lds);
    hipLaunchKernelGGL(kernel, grid, block, lds, c->stream, pack, c->gg, tm, ipb, ncodes);
  });
  return 0;
}

// the matrix-pipe level kernel takes gathering launches (site repeats) whose inner children are entry-contiguous
// (the rule unless PLL_AMD_NO_GENERIC_AOS=1), states_padded = 20
static bool lean_serves(const pllgpu_ctx *c, const OpPack &pack, unsigned nops, unsigned kind, bool gather)
{
  if (!gather) return kind == 2; // tip x tip: 204 us against the FMA kernel's 251 for C3's 32 cherries (same box)
  if (c->gg.SP != 20u) return false;
  for (unsigned i = 0; i < nops; ++i)
  {
    const unsigned lay = pack.ops[i].layout;
    if (kind == 0 && !(lay & kAosLeft)) return false;
    if (kind != 2 && !(lay & kAosRight)) return false;
  }
  return true;
}

static int launch_partials(pllgpu_ctx *c, const OpPack &pack, unsigned nops, unsigned maxent, unsigned kind, bool gather)
{
  if (c->dna_fast)
    launch_dna(c, pack, nops, maxent, kind, gather);
  else if (c->use_mfma)
    return launch_mfma(c, pack, nops, maxent, kind, gather);
  else if (c->lean && (kind == 0 || c->tipmap_set) && lean_serves(c, pack, nops, kind, gather))
    return launch_lean(c, pack, nops, maxent, kind, gather);
  else
    with_ich(c->ich, [&](auto ICH) { launch_generic<ICH()>(c, pack, nops, maxent, kind, gather); });
  return 0;
}

#include "fusion_plan.h"
#include "chain_plan.h"
#include "subtree_plan.h"

// matrices about to change: indices[0..count) if given, else [first, first + count)
struct MatrixSet
{
  const unsigned *indices;
  unsigned first, count;
  bool has(unsigned m) const
  {
    if (!indices) return m - first < count;
    for (unsigned i = 0; i < count; ++i)
      if (indices[i] == m) return true;
    return false;
  }
  bool read_by(const pllgpu_op_t &o) const { return has(o.left_matrix) || has(o.right_matrix); }
};

static bool held_work_reads_matrices(const pllgpu_ctx *c, const MatrixSet &ms)
{
  for (const pllgpu_op_t &o : c->deferred)
    if (ms.read_by(o)) return true;
  if (c->chain_held && c->plan)
    for (const pllgpu_op_t &o : c->plan->key)
      if (ms.read_by(o)) return true;
  return false;
}

static void set_pending(pllgpu_ctx *c, const ChainPlan *pl, bool deep)
{
  c->pending = deep ? pl->subtrees : pl->cherries;
  c->pending_deep = deep;
  c->pending_plan = pl;
  c->pending_mats_kept = false;
}

static void drop_pending(pllgpu_ctx *c)
{
  c->pending.clear();
  c->pending_deep = false;
  c->pending_plan = nullptr;
  c->pending_mats_kept = false;
}

// is this CLV one that the lean tree launch left unstored
static bool clv_is_pending(const pllgpu_ctx *c, unsigned clv)
{
  for (const pllgpu_op_t &o : c->pending)
    if (o.parent_clv == clv) return true;
  return false;
}

// The matrices the pending ops read, as they are now, into slots of their own: one launch of 2 x 32 or 2 x 56 blocks, 32
// or 56 KB for 4 states x 4 rates. Once per step at the most - from then on no change of a matrix concerns what is pending.
struct MatrixCopies
{
  unsigned short src[2 * kMaxPending];
};
__global__ void k_keep_matrices(const double *__restrict__ pmat, double *__restrict__ kept, MatrixCopies mc, unsigned stride)
{
  const double *s = pmat + (size_t)mc.src[blockIdx.x] * stride;
  double *d = kept + (size_t)blockIdx.x * stride;
  for (unsigned i = threadIdx.x; i < stride; i += blockDim.x) d[i] = s[i];
}

static int keep_pending_matrices(pllgpu_ctx *c)
{
  if (c->pending.empty() || c->pending_mats_kept) return 0;
  const unsigned n = (unsigned)c->pending.size();
  MatrixCopies mc;
  if (2u * n > sizeof mc.src / sizeof mc.src[0] || c->geo.prob_matrices > 65535u) return materialise_pending(c); // (cannot happen: 32 or 56 ops)
  for (unsigned i = 0; i < n; ++i)
  {
    mc.src[2 * i] = (unsigned short)c->pending[i].left_matrix;
    mc.src[2 * i + 1] = (unsigned short)c->pending[i].right_matrix;
  }
  if (int rc = c->pending_mats.ensure(c->pm_stride * 2u * n)) return rc;
  hipLaunchKernelGGL(k_keep_matrices, dim3(2u * n), dim3(64), 0, c->stream, c->pmat.p, c->pending_mats.p, mc, (unsigned)c->pm_stride);
  if (int rc = launch_status()) return rc;
  c->pending_mats_kept = true;
  return 0;
}

// Matrices are about to be overwritten, in stream order behind everything launched so far. Held work that reads one of
// them goes out first, with the old matrix. Pending CLVs that read one are NOT stored for it: the usual next call is the
// plan's own list again, which drops them - they keep copies of their matrices instead.
static int matrices_change(pllgpu_ctx *c, const unsigned *indices, unsigned first, unsigned count)
{
  if (!HOLDS_WORK(c) && c->pending.empty()) return 0;
  const MatrixSet ms{indices, first, count};
  if (HOLDS_WORK(c) && held_work_reads_matrices(c, ms))
    if (int rc = flush_deferred(c, true)) return rc;
  if (!c->pending.empty() && !c->pending_mats_kept)
    for (const pllgpu_op_t &o : c->pending)
      if (ms.read_by(o)) return keep_pending_matrices(c);
  return 0;
}

// Store the pending tip x tip parents: ordinary updates through the level path (k_partials_dna<tip, tip>, the arithmetic
// of dna_cherry: the bits the full launch stores), on the context's stream, from the codes as they are on the device and
// the matrices as they are there or as they were kept - those of the step, since nothing that changes them gets past
// matrices_change or this. The kept plan is not touched; the counters of the last update call stay what they were, the
// launch is counted. On an error they stay pending.
// A deep pending set - the 56 ops of eight complete groups, seven by seven as ChainPlan::subtrees lists them - is stored by
// the seven-op group launch in its full form (k_partials_dna_cc<CK_FCC, CK_FCC>: what the two-launch route stores), its
// descriptors resolved again here like the others'.
static int materialise_pending_groups(pllgpu_ctx *c)
{
  const size_t ngroups = c->pending.size() / 7u;
  if (c->pending.size() != ngroups * 7u || ngroups == 0 || ngroups > (size_t)kMaxCCGroups) return fail(PLLGPU_ERUNTIME, "pending groups out of shape");
  CCPack pack;
  memset(&pack, 0, sizeof pack);
  for (size_t gi = 0; gi < ngroups; ++gi)
  {
    CCGroup &cg = pack.g[gi];
    TOp *tops[7] = {&cg.aa, &cg.ab, nullptr, &cg.ba, &cg.bb, nullptr, nullptr};
    FOp *fops[7] = {nullptr, nullptr, &cg.a, nullptr, nullptr, &cg.b, &cg.p};
    for (size_t k = 0; k < 7u; ++k)
    {
      const size_t i = gi * 7u + k;
      DevOp d;
      if (int rc = resolve_op(c, c->pending[i], d)) return rc; // (the buffers exist: the plan resolved them)
      if (c->pending_mats_kept)
      {
        d.lmat = c->pending_mats.p + (2 * i) * c->pm_stride;
        d.rmat = c->pending_mats.p + (2 * i + 1) * c->pm_stride;
      }
      if (tops[k])
        to_top(d, *tops[k]);
      else
        to_fop(d, *fops[k]);
    }
  }
  if (int rc = launch_cc(c, pack, (unsigned)ngroups, c->pending[0].parent_entries, CK_FCC, CK_FCC)) return rc;
  ++c->last_launches;
  if (int rc = launch_status()) return rc;
  drop_pending(c);
  return 0;
}

static int materialise_pending(pllgpu_ctx *c)
{
  if (c->pending.empty()) return 0;
  if (c->pending_deep) return materialise_pending_groups(c);
  OpPack pack;
  unsigned nops = 0, maxent = 0;
  auto launch = [&]() -> int {
    if (!nops) return 0;
    if (int rc = launch_partials(c, pack, nops, maxent, 2, false)) return rc;
    ++c->last_launches;
    nops = maxent = 0;
    return 0;
  };
  for (size_t i = 0; i < c->pending.size(); ++i)
  {
    const pllgpu_op_t &o = c->pending[i];
    DevOp &d = pack.ops[nops];
    if (int rc = resolve_op(c, o, d)) return rc; // (the buffers exist: the plan resolved them)
    if (c->pending_mats_kept)
    {
      d.lmat = c->pending_mats.p + (2 * i) * c->pm_stride;
      d.rmat = c->pending_mats.p + (2 * i + 1) * c->pm_stride;
    }
    maxent = std::max(maxent, o.parent_entries);
    if (++nops == (unsigned)kMaxOpsPerLaunch)
      if (int rc = launch()) return rc;
  }
  if (int rc = launch()) return rc;
  if (int rc = launch_status()) return rc;
  drop_pending(c);
  return 0;
}

// for calls that read the two ends of an edge (or the one end of a root) and nothing else
static int materialise_if_an_end_is_pending(pllgpu_ctx *c, const pllgpu_edge_t *ed, bool is_root)
{
  if (c->pending.empty()) return 0;
  if (clv_is_pending(c, ed->parent_clv) || (!is_root && !ed->child_is_tip && clv_is_pending(c, ed->child_clv))) return materialise_pending(c);
  return 0;
}

// launch the held ops as ordinary updates (they are mutually independent: one level)
// keep_pending: for a caller that neither reads a CLV nor changes an input of one - what is pending stays, and a held whole
// traversal leaves its tip x tip parents pending as well
static int flush_deferred(pllgpu_ctx *c, bool keep_pending)
{
  if (!keep_pending)
    if (int rc = materialise_pending(c)) return rc;
  if (int rc = launch_held_chains(c, keep_pending)) return rc;
  std::vector<pllgpu_op_t> ops;
  ops.swap(c->deferred);
  for (unsigned kind = 0; kind < 3; ++kind)
  {
    OpPack pack;
    unsigned nops = 0, maxent = 0;
    for (const pllgpu_op_t &o : ops)
    {
      const unsigned tips = ((o.flags & PLLGPU_OP_LEFT_TIP) ? 1u : 0u) + ((o.flags & PLLGPU_OP_RIGHT_TIP) ? 1u : 0u);
      if (tips != kind) continue;
      if (int rc = resolve_op(c, o, pack.ops[nops])) return rc;
      maxent = std::max(maxent, o.parent_entries);
      ++nops;
    }
    if (!nops) continue;
    if (int rc = launch_partials(c, pack, nops, maxent, kind, false)) return rc;
    ++c->last_launches;
  }
  return launch_status();
}

// ---- the level scheduler: plan the list and launch it (every launch through emit_launch(), so that a plan being
// recorded keeps it). The steps below run in this order; each resolves its ops (resolve_op creates the buffers) and
// counts their bytes where it forms their launch.
static void dissolve_group(std::vector<Role> &role, const FusedGroup &g)
{
  role[g.p] = Role::Plain;
  if (g.a >= 0) role[g.a] = Role::Plain;
  if (g.b >= 0) role[g.b] = Role::Plain;
}

// of the groups the 4x4 planner knows, the other shapes have one: both children cherries
static void keep_cherry_pairs(std::vector<Role> &role, std::vector<FusedGroup> &groups)
{
  std::vector<FusedGroup> keep;
  for (const FusedGroup &gq : groups)
    if (gq.lk == CK_FTT && gq.rk == CK_FTT && gq.a >= 0 && gq.b >= 0)
      keep.push_back(gq);
    else
      dissolve_group(role, gq);
  groups.swap(keep);
}

// site repeats (4x4 kernels): an uncompressed op over two GATHERING inner x inner ops of the level below, all four
// of their children class-compressed, is evaluated with them (kernels_dna.h: k_partials_dna_gg). Such an op may
// have been taken as a producer by the op above it; that group gives way (its parent is usually one of the last
// level's ops, which then wait for the edge evaluation).
static void plan_gg_groups(const pllgpu_ctx *c, const pllgpu_op_t *ops, unsigned count, std::vector<Role> &role, std::vector<FusedGroup> &groups)
{
  std::vector<int> producer(c->geo.nodes, -1), pl(count, -1), pr(count, -1);
  for (unsigned q = 0; q < count; ++q)
  {
    if (!(ops[q].flags & PLLGPU_OP_LEFT_TIP)) pl[q] = producer[ops[q].left_clv];
    if (!(ops[q].flags & PLLGPU_OP_RIGHT_TIP)) pr[q] = producer[ops[q].right_clv];
    producer[ops[q].parent_clv] = (int)q;
  }
  auto gathering = [&](int x, int pscal, const pllgpu_op_t &P, unsigned L) {
    if (x < 0 || role[x] != Role::Plain) return false;
    const pllgpu_op_t &o = ops[x];
    return o.level == L && (o.flags & PLLGPU_OP_GATHER) && !(o.flags & (PLLGPU_OP_LEFT_TIP | PLLGPU_OP_RIGHT_TIP)) &&
           o.parent_entries == P.parent_entries && o.parent_entries == c->geo.sites_alloc && o.parent_scaler == pscal &&
           c->ids[o.left_clv] && c->ids[o.right_clv];
  };
  for (unsigned q = 0; q < count; ++q)
  {
    const pllgpu_op_t &P = ops[q];
    if ((P.flags & (PLLGPU_OP_GATHER | PLLGPU_OP_LEFT_TIP | PLLGPU_OP_RIGHT_TIP)) || P.level == 0 || role[q] == Role::GroupParent) continue;
    const unsigned L = P.level - 1;
    if (P.war_level >= (int)L || pl[q] == pr[q]) continue;
    if (!gathering(pl[q], P.left_scaler, P, L) || !gathering(pr[q], P.right_scaler, P, L)) continue;
    if (role[q] == Role::GroupProducer)
    {
      // dissolve the group that took P as a producer
      for (size_t gi = 0; gi < groups.size(); ++gi)
        if ((groups[gi].a == (int)q || groups[gi].b == (int)q) && groups[gi].lk != CK_FCC && groups[gi].rk != CK_FCC)
        {
          dissolve_group(role, groups[gi]);
          groups.erase(groups.begin() + gi);
          break;
        }
      if (role[q] != Role::Plain) continue; // (a cherry-cherry side: leave it)
    }
    FusedGroup gq;
    gq.p = q;
    gq.a = pl[q];
    gq.b = pr[q];
    gq.lk = gq.rk = CK_FGG;
    gq.level = L;
    role[q] = Role::GroupParent;
    role[gq.a] = role[gq.b] = Role::GroupProducer;
    groups.push_back(gq);
  }
}

// tail fusion: the plain ops of the last level (at most two: the ends of the edge a caller evaluates
// next) are accepted but not launched yet - Role::HeldTail
static void hold_tail(pllgpu_ctx *c, const pllgpu_op_t *ops, unsigned count, std::vector<Role> &role)
{
  const unsigned top = ops[count - 1].level;
  unsigned n = 0;
  bool ok = true;
  for (unsigned o = 0; o < count && ok; ++o)
    if (ops[o].level == top)
    {
      if (role[o] == Role::GroupParent) continue; // a group parent hoisted away from this level
      ok = role[o] == Role::Plain && !(ops[o].flags & PLLGPU_OP_GATHER) && ops[o].parent_entries == c->geo.sites_alloc && ++n <= 2;
    }
  for (unsigned o = 0; o < count && ok; ++o)
    if (ops[o].level == top && role[o] == Role::Plain)
    {
      role[o] = Role::HeldTail;
      c->deferred.push_back(ops[o]);
      c->last_bytes += op_traffic(c, ops[o], true, true);
    }
}

// site repeats: every all-tip subtree of up to three ops' depth in one launch, before the levels (Role::SubtreeMember)
static int launch_subtree_ops(pllgpu_ctx *c, const pllgpu_op_t *ops, unsigned count, std::vector<Role> &role)
{
  unsigned nsub = 0, sub_entries = 0;
  if (int rc = plan_subtrees(c, ops, count, role, nsub, sub_entries)) return rc;
  if (!nsub) return 0;
  return emit_launch(c, [c, items = c->sub_build]() {
    if (int rc = upload_subtrees(c, items)) return rc;
    launch_subtrees(c, (unsigned)items.size());
    return 0;
  }, (nsub + (unsigned)kSubItemsPerLaunch - 1) / (unsigned)kSubItemsPerLaunch);
}

// plain ops [i, j) of one level: one launch group per (child kinds, gather) in packs of kMaxOpsPerLaunch
static int launch_plain_packs(pllgpu_ctx *c, const pllgpu_op_t *ops, unsigned i, unsigned j, const std::vector<Role> &role)
{
  for (unsigned kind = 0; kind < 3; ++kind)
    for (unsigned ga = 0; ga < 2; ++ga)
    {
      OpPack pack;
      unsigned nops = 0, maxent = 0;
      auto flush = [&]() -> int {
        if (!nops) return 0;
        const bool gather = ga != 0;
        const int rc = emit_launch(c, [c, pack, nops, maxent, kind, gather]() { return launch_partials(c, pack, nops, maxent, kind, gather); });
        nops = 0;
        maxent = 0;
        return rc;
      };
      for (unsigned o = i; o < j; ++o)
      {
        const unsigned f = ops[o].flags;
        const unsigned tips = ((f & PLLGPU_OP_LEFT_TIP) ? 1u : 0u) + ((f & PLLGPU_OP_RIGHT_TIP) ? 1u : 0u);
        if ((f & PLLGPU_OP_RIGHT_TIP) && !(f & PLLGPU_OP_LEFT_TIP))
          return fail(PLLGPU_EINVAL, "tip-inner operations must carry the tip as the left child");
        if (role[o] != Role::Plain || tips != kind || ((f & PLLGPU_OP_GATHER) ? 1u : 0u) != ga) continue;
        if (ops[o].parent_entries == 0) continue;
        if (int rc = resolve_op(c, ops[o], pack.ops[nops])) return rc;
        c->last_bytes += op_traffic(c, ops[o], true, true);
        maxent = std::max(maxent, ops[o].parent_entries);
        if (++nops == (unsigned)kMaxOpsPerLaunch)
          if (int rc = flush()) return rc;
      }
      if (int rc = flush()) return rc;
    }
  return 0;
}

// cherry-cherry groups (kind CK_FCC on at least one side) have their own descriptor and kernel
static int launch_cc_groups(pllgpu_ctx *c, const pllgpu_op_t *ops, const std::vector<FusedGroup> &groups, size_t g0, size_t g1)
{
  std::vector<CCLaunch> ccl;
  if (int rc = build_cc_launches(c, ops, groups, g0, g1, ccl)) return rc;
  for (const CCLaunch &l : ccl)
    if (int rc = emit_launch(c, [c, l]() { return launch_cc(c, l.pack, l.n, l.entries, l.lk, CK_FCC); })) return rc;
  return 0;
}

// groups over two gathering producers (site repeats)
static int launch_gg_packs(pllgpu_ctx *c, const pllgpu_op_t *ops, const std::vector<FusedGroup> &groups, size_t g0, size_t g1)
{
  GGPack gp;
  unsigned n = 0, entries = 0;
  auto flush = [&]() -> int {
    if (!n) return 0;
    const int rc = emit_launch(c, [c, gp, n, entries]() {
      launch_gg(c, gp, n, entries);
      return 0;
    });
    n = 0;
    return rc;
  };
  for (size_t gi = g0; gi < g1; ++gi)
  {
    const FusedGroup &gq = groups[gi];
    if (gq.lk != CK_FGG) continue;
    const pllgpu_op_t &P = ops[gq.p];
    if (P.parent_entries == 0) continue;
    if (n && P.parent_entries != entries)
      if (int rc = flush()) return rc;
    entries = P.parent_entries;
    GGroup &gg = gp.g[n];
    memset(&gg, 0, sizeof gg);
    DevOp d;
    if (int rc = resolve_op(c, ops[gq.a], gg.a)) return rc;
    if (int rc = resolve_op(c, ops[gq.b], gg.b)) return rc;
    if (int rc = resolve_op(c, P, d)) return rc;
    to_fop(d, gg.p);
    c->last_bytes += op_traffic(c, ops[gq.a], true, true) + op_traffic(c, ops[gq.b], true, true) + op_traffic(c, P, false, false);
    if (++n == (unsigned)kMaxGGroups)
      if (int rc = flush()) return rc;
  }
  return flush();
}

// the other fused groups [g0, g1) executing at one level, one launch per pair of child kinds
static int launch_fused_packs(pllgpu_ctx *c, const pllgpu_op_t *ops, const std::vector<FusedGroup> &groups, size_t g0, size_t g1)
{
  for (int lk = 0; lk <= CK_FII; ++lk)
    for (int rk = lk; rk <= CK_FII; ++rk)
    {
      FusePack pack;
      unsigned n = 0, entries = 0;
      auto flush = [&]() -> int {
        if (!n) return 0;
        const int rc = c->dna_fast ? emit_launch(c, [c, pack, n, entries, lk, rk]() { return launch_fused(c, pack, n, entries, lk, rk); })
                                   : emit_launch(c, [c, pack, n, entries]() { return launch_mfma_cc(c, pack, n, entries); });
        n = 0;
        return rc;
      };
      for (size_t gi = g0; gi < g1; ++gi)
      {
        FusedGroup g = groups[gi];
        if (g.lk == CK_FCC || g.rk == CK_FCC || g.lk == CK_FGG) continue; // launched by launch_cc_groups / launch_gg_packs
        const bool swap = g.lk > g.rk; // canonical order: the "smaller" kind on the left
        if ((swap ? g.rk : g.lk) != lk || (swap ? g.lk : g.rk) != rk) continue;
        const pllgpu_op_t &P = ops[g.p];
        if (P.parent_entries == 0) continue;
        if (n && P.parent_entries != entries)
          if (int rc = flush()) return rc;
        entries = P.parent_entries;
        DevOp dp, da, db;
        FGroup &fg = pack.g[n];
        memset(&fg, 0, sizeof fg);
        // producers first: their parent buffers must exist before P's children are resolved
        if (g.a >= 0)
        {
          if (int rc = resolve_op(c, ops[g.a], da)) return rc;
          c->last_bytes += op_traffic(c, ops[g.a], true, true);
        }
        if (g.b >= 0)
        {
          if (int rc = resolve_op(c, ops[g.b], db)) return rc;
          c->last_bytes += op_traffic(c, ops[g.b], true, true);
        }
        if (int rc = resolve_op(c, P, dp)) return rc;
        c->last_bytes += op_traffic(c, P, g.a < 0, g.b < 0);
        to_fop(dp, fg.p);
        if (g.a >= 0) to_fop(da, fg.a);
        if (g.b >= 0) to_fop(db, fg.b);
        if (swap)
        {
          std::swap(fg.p.left, fg.p.right);
          std::swap(fg.p.ltip, fg.p.rtip);
          std::swap(fg.p.lscaler, fg.p.rscaler);
          std::swap(fg.p.lmat, fg.p.rmat);
          std::swap(fg.a, fg.b);
        }
        if (++n == (unsigned)kMaxGroups)
          if (int rc = flush()) return rc;
      }
      if (int rc = flush()) return rc;
    }
  return 0;
}

static int plan_and_launch_levels(pllgpu_ctx *c, const pllgpu_op_t *ops, unsigned count)
{
  c->launch_rc = 0;
  std::vector<Role> role;
  std::vector<FusedGroup> groups;
  // the groups look their cherries' scaling decisions up in a table over all pairs of tip codes: only for a sane number of codes
  const bool cherry_groups = c->fuse_mfma && c->tipmap_set && c->tip_ncodes <= 32u;
  const bool generic_groups = cherry_groups;
  plan_fusion(c->fuse || generic_groups, c->fuse_cc, c->geo.nodes, ops, count, role, groups);
  if (generic_groups) keep_cherry_pairs(role, groups);
  if (c->dna_fast && c->fuse && c->fuse_gg) plan_gg_groups(c, ops, count, role, groups);
  if (c->defer_tail && count) hold_tail(c, ops, count, role);
  if (int rc = launch_subtree_ops(c, ops, count, role)) return rc;
  size_t gi_sorted = 0;
  if (!groups.empty())
    sort_groups_by_level(groups);
  unsigned i = 0;
  const unsigned last_level = count ? ops[count - 1].level : 0;
  for (unsigned level = 0; level <= last_level; ++level)
  {
    // [i, j) = the ops of this dependency level
    unsigned j = i;
    while (j < count && ops[j].level == level) ++j;
    if (int rc = launch_plain_packs(c, ops, i, j, role)) return rc;
    // [g0, gi_sorted) = the fused groups executing at this level
    const size_t g0 = gi_sorted;
    while (gi_sorted < groups.size() && groups[gi_sorted].level == level) ++gi_sorted;
    if (int rc = launch_cc_groups(c, ops, groups, g0, gi_sorted)) return rc;
    if (int rc = launch_gg_packs(c, ops, groups, g0, gi_sorted)) return rc;
    if (int rc = launch_fused_packs(c, ops, groups, g0, gi_sorted)) return rc;
    i = j;
  }
  return launch_status();
}

extern "C" int pllgpu_update_partials(pllgpu_ctx_t *c, const pllgpu_op_t *ops, unsigned count)
{
  CHECK_CTX_KEEP(c);
  // the kept plan's own list again (what try_chain_plan will replay) recomputes every pending CLV: they are dropped, not
  // stored. However the held plan is resolved later, it stores them or leaves them pending again. Any other list may read
  // or overwrite them: stored first. Compared BEFORE anything is flushed.
  const bool replay = c->plan && c->chains && c->fuse && !c->any_aos && c->plan->epoch == c->alloc_epoch && c->plan->key.size() == count &&
                      memcmp(c->plan->key.data(), ops, count * sizeof(pllgpu_op_t)) == 0;
  // Such a caller read nothing since the plan's last launch: a loop. Its next one-launch evaluation may leave the whole
  // 8-tip groups unstored (k_edge_dna_tree<TopsOnly>) - decided here, for last_bytes is read before the evaluation.
  c->tree_deep = replay && c->pending_plan == c->plan && !c->pending.empty() && c->plan->tree && use_deep_tree(c, c->plan->entries);
  if (replay && c->pending_plan == c->plan) drop_pending(c);
  // (the same list while it is still held: the traversal goes out, and what it would store only to be recomputed below
  // stays unstored)
  if (HOLDS_WORK(c) || !c->pending.empty())
    if (int rc = flush_deferred(c, replay && c->pending.empty())) return rc;
  if (replay && c->pending_plan == c->plan) drop_pending(c);
  c->last_launches = 0;
  c->last_bytes = 0.0;
  {
    bool used = false;
    if (int rc = try_chain_plan(c, ops, count, used)) return rc;
    if (used) return 0;
    c->last_bytes = 0.0;
  }
  if (c->plan_cache)
  {
    const unsigned long long epoch = c->alloc_epoch;
    for (LevelPlan *lp : c->level_plans)
      if (lp->alloc_epoch == epoch && lp->maps_epoch == c->maps_epoch && lp->key.size() == count &&
          memcmp(lp->key.data(), ops, count * sizeof(pllgpu_op_t)) == 0)
      {
        // the same list, nothing it points at has moved: the same launches
        for (const auto &a : lp->aos) c->clv_aos[a.first] = a.second;
        if (lp->any_aos) c->any_aos = true;
        c->deferred = lp->deferred;
        c->launch_rc = 0;
        for (const auto &fn : lp->launches)
          if (int rc = fn()) c->launch_rc = rc;
        ++c->plan_replays;
        c->last_launches = lp->nlaunches;
        c->last_bytes = lp->bytes;
        lp->used = ++c->plan_stamp;
        return c->launch_rc ? c->launch_rc : launch_status();
      }
  }
  LevelPlan *lp = c->plan_cache ? new LevelPlan() : nullptr;
  c->recording = lp;
  const int rc = plan_and_launch_levels(c, ops, count);
  c->recording = nullptr;
  if (!lp) return rc;
  if (rc)
  {
    delete lp;
    return rc;
  }
  lp->key.assign(ops, ops + count);
  lp->alloc_epoch = c->alloc_epoch; // after the planning: it may have allocated
  lp->maps_epoch = c->maps_epoch;
  lp->deferred = c->deferred;
  for (unsigned i = 0; i < count; ++i) lp->aos.emplace_back(ops[i].parent_clv, c->clv_aos[ops[i].parent_clv]);
  lp->any_aos = c->any_aos;
  lp->nlaunches = c->last_launches;
  lp->bytes = c->last_bytes;
  lp->used = ++c->plan_stamp;
  if (c->level_plans.size() >= kLevelPlans)
  {
    size_t victim = 0;
    for (size_t i = 1; i < c->level_plans.size(); ++i)
      if (c->level_plans[i]->used < c->level_plans[victim]->used) victim = i;
    delete c->level_plans[victim];
    c->level_plans[victim] = lp;
  }
  else
    c->level_plans.push_back(lp);
  return 0;
}

extern "C" double pllgpu_last_algorithmic_bytes(const pllgpu_ctx_t *c) { return c ? c->last_bytes : 0.0; }
extern "C" unsigned pllgpu_pending_clvs(const pllgpu_ctx_t *c) { return c ? (unsigned)c->pending.size() : 0u; }

// ---- log-likelihood ----------------------------------------------------------------------------
template <int ICH>
static void launch_edge_generic(pllgpu_ctx *c, const DevEdge &e, unsigned blocks, unsigned tpw, bool ctip, bool gather)
{
  const unsigned long long *tm = tipmap_ptr(c);
  with_bools(ctip, gather, [&](auto CT, auto GA) {
    hipLaunchKernelGGL((k_edge_tiled<ICH, CT(), GA()>), dim3(blocks), dim3(tiled_threads(c)), 0, c->stream, e, c->gg, tm, tpw);
  });
}

// the tail-fused evaluation: kinds of the two ends and the descriptors of the held ops
struct TailCall
{
  FGroup g;
  int kp, kc;
};

static int launch_edge_tail(pllgpu_ctx *c, const DevEdge &e, const TailCall &t, unsigned blocks, unsigned tpw)
{
  const bool known = with_kind_pair(
      t.kp, t.kc,
      [&](auto KP, auto KC) {
        hipLaunchKernelGGL((k_edge_dna_tail<KP(), KC()>), dim3(blocks), dim3(256), 0, c->stream, e, t.g, c->gg.scale_mode, tpw);
      },
      KindPair<CK_INNER, CK_FTT>(), KindPair<CK_INNER, CK_FTI>(), KindPair<CK_INNER, CK_FII>(),
      KindPair<CK_FTT, CK_INNER>(), KindPair<CK_FTT, CK_TIP>(), KindPair<CK_FTT, CK_FTT>(), KindPair<CK_FTT, CK_FTI>(), KindPair<CK_FTT, CK_FII>(),
      KindPair<CK_FTI, CK_INNER>(), KindPair<CK_FTI, CK_TIP>(), KindPair<CK_FTI, CK_FTT>(), KindPair<CK_FTI, CK_FTI>(), KindPair<CK_FTI, CK_FII>(),
      KindPair<CK_FII, CK_INNER>(), KindPair<CK_FII, CK_TIP>(), KindPair<CK_FII, CK_FTT>(), KindPair<CK_FII, CK_FTI>(), KindPair<CK_FII, CK_FII>());
  if (!known) return fail(PLLGPU_EINVAL, "no tail kernel for end kinds (%d, %d)", t.kp, t.kc);
  return 0;
}

// chain tail (kernels_dna.h: k_edge_dna_chain): the two ends of the edge as chains - held ones, or chains of
// no steps around a CLV / tip that is in HBM
struct ChainTailCall
{
  ChainHead hp, hc;
  unsigned variant;
  bool in_kernarg;
  ChainPack pack; // in_kernarg: heads[0] = hp, heads[1] = hc and their steps
  const TreePack *tree = nullptr; // the held plan is a whole traversal (ChainPlan::tree): k_edge_dna_tree, nothing above is read
  bool lean = false;              // ... in the form that leaves the 32 tip x tip parents unstored (pllgpu_ctx::pending)
  bool deep = false;              // ... and the rest of the eight groups as well (lean too)
};

static void launch_edge_chain(pllgpu_ctx *c, const DevEdge &e, const ChainTailCall &t)
{
  const ChainPlan &pl = *c->plan;
  dim3 grid((pl.entries + 63) / 64), block(256);
  if (t.tree) // a workgroup of eight waves per tile, tiles in the XCD-aware order
  {
    auto go = [&](auto ST) {
      hipLaunchKernelGGL(k_edge_dna_tree<ST()>, xcd_grid(grid.x, 1), dim3(512), 0, c->stream, e, *t.tree, pl.entries, c->gg.scale_mode, c->xcd_order);
    };
    if (t.deep)
      go(std::integral_constant<TreeStores, TreeStores::TopsOnly>());
    else if (t.lean)
      go(std::integral_constant<TreeStores, TreeStores::NoCherries>());
    else
      go(std::integral_constant<TreeStores, TreeStores::All>());
  }
  else if (t.in_kernarg)
    with_chain_variant(c->gg.scale_mode, t.variant, [&](auto SMV, auto C0, auto S1, auto C1) {
      hipLaunchKernelGGL((k_edge_dna_chain_pack<SMV(), C0(), S1(), C1()>), grid, block, 0, c->stream, e, t.pack, pl.entries);
    });
  else
  {
    const ChainStepLoad *lp;
    const ChainStepOp *op;
    chain_steps_on_device(c, pl, lp, op);
    with_chain_variant(c->gg.scale_mode, t.variant, [&](auto SMV, auto C0, auto S1, auto C1) {
      hipLaunchKernelGGL((k_edge_dna_chain<SMV(), C0(), S1(), C1()>), grid, block, 0, c->stream, e, t.hp, t.hc, lp, op, pl.entries);
    });
  }
}

// 33..64 states: P x on the matrix pipe (kernels_mfma.h: k_edge_mfma), one rate category per workgroup
static int launch_edge_mfma(pllgpu_ctx *c, DevEdge &e, bool ctip, bool gather)
{
  const pllgpu_geometry_t &g = c->geo;
  const unsigned items = (g.sites + 31) / 32, R = c->gg.R;
  // a workgroup's life is a chain of round trips (matrix, child, parent, ticket, partials, block sum: ~30 us at C5's
  // size) around 3 us of MFMAs per item, and two workgroups fit a CU: ONE round of at most 512 workgroups - C5's 625
  // items as 628 workgroups of one item per wave took two rounds, 67 us; as 316 of two items per wave 3x us
  const unsigned max_ib = std::max(1u, 512u / R);
  const unsigned ipw = std::max(1u, (items + 4u * max_ib - 1) / (4u * max_ib));
  const unsigned nib = (items + 4u * ipw - 1) / (4u * ipw);
  const unsigned blocks = nib * R;
  const unsigned pstride = (g.sites + 63u) & ~63u;
  if (c->block_sums.ensure(std::max<size_t>(4096, blocks)) || c->edge_partials.ensure((size_t)R * 4u * pstride)) return PLLGPU_ENOMEM;
  if (c->edge_tickets.cap < nib)
  {
    if (c->edge_tickets.ensure(std::max(1024u, nib))) return PLLGPU_ENOMEM;
    HIP_TRY(hipMemsetAsync(c->edge_tickets.p, 0, c->edge_tickets.cap * sizeof(unsigned), c->stream));
  }
  e.block_sums = c->block_sums.p;
  const size_t lds = (kFragArray + 64) * sizeof(double);
  const unsigned long long *tm = tipmap_ptr(c);
  with_bools(ctip, gather, [&](auto CT, auto GA) {
    hipLaunchKernelGGL((k_edge_mfma<CT(), GA()>), dim3(blocks), dim3(256), lds, c->stream, e, c->gg, tm, ipw, c->edge_partials.p, pstride, c->edge_tickets.p);
  });
  return 0;
}

// The tile walk of every kernel whose grid is cut by the site count alone (the edge evaluation, each batched call, the
// per-site tables): the grid's x axis and the tiles each wave or workgroup walks, at most max_blocks workgroups' worth.
// The order of every sum over the sites follows from it, so it depends on the site count and the shape alone. Every such
// walk goes through this function; the three bounds in use are named here and in qgradient_walk.
struct TileWalk
{
  unsigned blocks, tiles_per;
};

constexpr unsigned kSumBlocks = 1024;   // kernels that sum over the sites: a slot per workgroup to add up
constexpr unsigned kTableBlocks = 4096; // kernels that leave a table per site (ancestral states, category likelihoods): a read
                                        // stream with a short store, one tile per wave as long as that is no more (kernels_dna.h, "Tiles per wave")

static TileWalk tile_walk(const pllgpu_ctx *c, unsigned max_blocks = kSumBlocks)
{
  const unsigned tiles = (c->geo.sites + 63) / 64;
  TileWalk w;
  if (c->dna_fast)
  {
    // 4 waves = 4 tiles per workgroup, tiles_per consecutive tiles per wave
    w.tiles_per = (tiles + 4 * max_blocks - 1) / (4 * max_blocks);
    w.blocks = (tiles + 4 * w.tiles_per - 1) / (4 * w.tiles_per);
  }
  else
  {
    // one tile per workgroup pass (the waves split its rate categories), tiles_per tiles per workgroup
    w.tiles_per = (tiles + max_blocks - 1) / max_blocks;
    w.blocks = (tiles + w.tiles_per - 1) / w.tiles_per;
  }
  return w;
}

// the evaluation's one launch: which kernel family takes it
static int launch_edge(pllgpu_ctx *c, DevEdge &e, bool ctip, bool gather, const TailCall *tail, const ChainTailCall *ctail)
{
  if (c->use_mfma && c->mfma_ng == 16 && !e.is_root) return launch_edge_mfma(c, e, ctip, gather);
  if (c->dna_fast && ctail)
  {
    launch_edge_chain(c, e, *ctail);
    ++c->last_launches;
    return 0;
  }
  const TileWalk w = tile_walk(c);
  if (c->dna_fast && tail)
  {
    if (int rc = launch_edge_tail(c, e, *tail, w.blocks, w.tiles_per)) return rc;
    ++c->last_launches;
  }
  else if (c->dna_fast)
    with_bools(ctip, gather, [&](auto CT, auto GA) {
      hipLaunchKernelGGL((k_edge_dna<CT(), GA()>), dim3(w.blocks), dim3(256), 0, c->stream, e, w.tiles_per);
    });
  else
    with_ich(c->ich, [&](auto ICH) { launch_edge_generic<ICH()>(c, e, w.blocks, w.tiles_per, ctip, gather); });
  return 0;
}

// what an evaluation reads besides its two ends: the model, the weights, the site count and the hand-off's form
static int fill_edge_model(pllgpu_ctx *c, DevEdge &e, const unsigned *freqs_indices)
{
  const pllgpu_geometry_t &g = c->geo;
  for (unsigned k = 0; k < g.rate_cats; ++k)
  {
    if (freqs_indices[k] >= g.rate_matrices) return fail(PLLGPU_EINVAL, "freqs_indices[%u] = %u out of range", k, freqs_indices[k]);
    e.fidx[k] = (unsigned char)freqs_indices[k];
  }
  e.freqs = c->freqs.p;
  e.rate_weights = c->rate_weights.p;
  e.prop_invar = c->prop_invar.p;
  e.pattern_weights = c->pattern_weights.p;
  e.invariant = c->invariant_set ? c->invariant.p : nullptr;
  e.sites = g.sites;
  e.per_rate = g.per_rate_scalers ? 1 : 0;
  e.fenced = c->fenced;
  return 0;
}

static int run_lnl(pllgpu_ctx *c, DevEdge &e, bool ctip, bool gather, const unsigned *freqs_indices,
                   double *persite_host, double *lnl_out, double *device_result = nullptr, const TailCall *tail = nullptr,
                   const ChainTailCall *ctail = nullptr)
{
  const pllgpu_geometry_t &g = c->geo;
  if (int rc = fill_edge_model(c, e, freqs_indices)) return rc;
  e.persite = persite_host ? c->persite.p : nullptr;
  e.block_sums = c->block_sums.p;
  e.counter = c->counter.p;
  e.result = device_result ? device_result : c->result_dev;
  if (c->seq_override != 0.0)
    e.sequence = c->seq_override; // a collective's step number: only meaningful in device_result
  else
  {
    c->seq += 1.0;
    e.sequence = c->seq;
  }
  if (int rc = launch_edge(c, e, ctip, gather, tail, ctail)) return rc;
  HIP_TRY(hipGetLastError());
  if (device_result) return 0; // asynchronous: the value stays on the device
  if (persite_host)
  {
    HIP_TRY(hipMemcpyAsync(persite_host, c->persite.p, g.sites * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  else
  {
    // the last workgroup stores {lnL, sequence} into mapped host memory
    if (int rc = wait_for_sequence(c, e.sequence)) return rc;
  }
  *lnl_out = c->result_host[0];
  return 0;
}

static int scaler_ptr(pllgpu_ctx *c, int idx, const unsigned *&out)
{
  out = nullptr;
  if (idx < 0) return 0;
  if ((unsigned)idx >= c->geo.scale_buffers || !c->scaler[idx].p)
    return fail(PLLGPU_EINVAL, "scale buffer %d unavailable on the device", idx);
  out = c->scaler[idx].p;
  return 0;
}

// Work that pllgpu_edge_loglikelihood has taken out of the held state (chain heads, deferred ops) in order
// to evaluate it inside the log-likelihood kernel. If the call fails before that kernel is launched the
// host layer has already marked those CLVs and scalers as device-side, so they must still be computed:
// the guard launches them as ordinary updates on every exit path that does not disarm it.
struct ClaimedWork
{
  pllgpu_ctx *c;
  int heads[2] = {-1, -1};
  bool tree = false; // the heads' whole plan was held (ChainPlan::tree): its groups first
  std::vector<pllgpu_op_t> ops;
  bool armed = false;
  explicit ClaimedWork(pllgpu_ctx *ctx) : c(ctx) {}
  void disarm() { armed = false; }
  ~ClaimedWork()
  {
    if (!armed) return;
    char keep[sizeof g_err];
    memcpy(keep, g_err, sizeof keep); // the error that brought us here is the one to report
    if (c->plan && tree)
    {
      c->tree_held = true;
      (void)launch_held_tree_groups(c);
    }
    if (c->plan)
      for (int h : heads)
        if (h >= 0)
        {
          launch_chain_heads(c, *c->plan, (unsigned)h, 1, c->plan->head_variant[h]);
          ++c->last_launches;
        }
    if (!ops.empty())
    {
      c->deferred.insert(c->deferred.end(), ops.begin(), ops.end());
      (void)flush_deferred(c);
    }
    (void)hipGetLastError();
    memcpy(g_err, keep, sizeof keep);
  }
};

// everything about an edge evaluation that can be checked without touching the held state
static int check_edge(const pllgpu_ctx *c, const pllgpu_edge_t *ed, const double *persite_host)
{
  const pllgpu_geometry_t &g = c->geo;
  if (ed->parent_clv >= g.nodes || ed->child_clv >= g.nodes || ed->matrix >= g.prob_matrices)
    return fail(PLLGPU_EINVAL, "edge references an index out of range");
  if (ed->parent_scaler >= (int)g.scale_buffers || ed->child_scaler >= (int)g.scale_buffers)
    return fail(PLLGPU_EINVAL, "edge references a scale buffer out of range");
  if (ed->device_result && persite_host) return fail(PLLGPU_EINVAL, "per-site values are not available from an asynchronous evaluation");
  if (ed->sequence != 0.0 && !ed->device_result) return fail(PLLGPU_EINVAL, "a caller-numbered evaluation needs device_result");
  if (ed->child_is_tip && (ed->child_clv >= g.tips || !c->tipchars[ed->child_clv].p))
    return fail(PLLGPU_EINVAL, "tip %u has no codes on the device", ed->child_clv);
  for (unsigned k = 0; k < g.rate_cats; ++k)
    if (ed->freqs_indices[k] >= g.rate_matrices) return fail(PLLGPU_EINVAL, "freqs_indices[%u] = %u out of range", k, ed->freqs_indices[k]);
  return 0;
}

// held chains: the heads of those that end in this edge's parent / child end (held_p / held_c, or -1) are claimed for
// the log-likelihood kernel; whatever else is held goes out as ordinary chain launches
static int claim_held_chains(pllgpu_ctx *c, const pllgpu_edge_t *ed, ClaimedWork &claimed, int &held_p, int &held_c)
{
  held_p = held_c = -1;
  if (!c->chain_held) return 0;
  const ChainPlan &pl = *c->plan;
  if (c->tree_held)
  {
    // a whole traversal is held: this evaluation takes it in one launch if it is of the edge between the two tops ...
    for (int h = 0; h < 2 && !ed->gather && !ed->child_is_tip; ++h)
      if (pl.head_top_clv[h] == ed->parent_clv && pl.head_top_scaler[h] == ed->parent_scaler && pl.head_top_clv[1 - h] == ed->child_clv &&
          pl.head_top_scaler[1 - h] == ed->child_scaler)
      {
        if (int rc = c->block_sums.ensure((pl.entries + 63) / 64)) return rc; // before anything is claimed
        c->chain_held = c->tree_held = false;
        held_p = claimed.heads[0] = h;
        held_c = claimed.heads[1] = 1 - h;
        claimed.tree = claimed.armed = true;
        return 0;
      }
    // ... any other edge meets today's plan: the groups go out, the chains stay held for the choice below
    if (int rc = launch_held_tree_groups(c)) return rc;
  }
  if (c->dna_fast && !ed->gather)
    for (size_t i = pl.held_from; i < pl.stages.size(); ++i)
      for (unsigned h = pl.stages[i].first_head; h < pl.stages[i].first_head + pl.stages[i].nchains; ++h)
      {
        if (pl.head_top_clv[h] == ed->parent_clv && pl.head_top_scaler[h] == ed->parent_scaler) held_p = (int)h;
        else if (!ed->child_is_tip && pl.head_top_clv[h] == ed->child_clv && pl.head_top_scaler[h] == ed->child_scaler) held_c = (int)h;
      }
  // a tail that would not fit its kernarg pack (try_chain_plan keeps such plans in memory: cannot happen
  // there; defensive): nothing is claimed, both chains go out as ordinary launches
  if ((held_p >= 0 || held_c >= 0) && pl.in_kernarg)
  {
    const unsigned np = held_p >= 0 ? pl.heads[held_p].nsteps + 1 : 1u, nc = held_c >= 0 ? pl.heads[held_c].nsteps + 1 : 1u;
    if (np + nc > (unsigned)kChainPackSteps) held_p = held_c = -1;
  }
  if (held_p < 0 && held_c < 0) return launch_held_chains(c);
  if (int rc = c->block_sums.ensure((pl.entries + 63) / 64)) return rc; // before anything is claimed
  // whatever else is held goes out as an ordinary chain launch
  c->chain_held = false;
  claimed.heads[0] = held_p;
  claimed.heads[1] = held_c;
  claimed.armed = true;
  for (size_t i = pl.held_from; i < pl.stages.size(); ++i)
    for (unsigned h = pl.stages[i].first_head; h < pl.stages[i].first_head + pl.stages[i].nchains; ++h)
      if ((int)h != held_p && (int)h != held_c)
      {
        launch_chain_heads(c, pl, h, 1, pl.stages[i].variant);
        ++c->last_launches;
      }
  return 0;
}

// held ops (tail fusion): if they produce an end of THIS edge they are evaluated inside the lnL
// kernel (use_tail, their descriptors and kinds in tail); whatever else is held goes out as ordinary updates first
static int claim_held_ops(pllgpu_ctx *c, const pllgpu_edge_t *ed, ClaimedWork &claimed, TailCall &tail, bool &use_tail)
{
  use_tail = false;
  if (c->deferred.empty()) return 0;
  int ia = -1, ib = -1;
  if (c->dna_fast && !ed->gather)
    for (size_t i = 0; i < c->deferred.size(); ++i)
    {
      const pllgpu_op_t &o = c->deferred[i];
      if (o.parent_clv == ed->parent_clv && o.parent_scaler == ed->parent_scaler) ia = (int)i;
      else if (!ed->child_is_tip && o.parent_clv == ed->child_clv && o.parent_scaler == ed->child_scaler) ib = (int)i;
    }
  if (ia < 0 && ib < 0) return flush_deferred(c);
  std::vector<pllgpu_op_t> held;
  held.swap(c->deferred);
  for (size_t i = 0; i < held.size(); ++i)
    if ((int)i != ia && (int)i != ib) c->deferred.push_back(held[i]);
  if (ia >= 0) claimed.ops.push_back(held[ia]);
  if (ib >= 0) claimed.ops.push_back(held[ib]);
  claimed.armed = true;
  if (!c->deferred.empty())
    if (int rc = flush_deferred(c)) return rc;
  memset(&tail.g, 0, sizeof tail.g);
  DevOp d;
  if (ia >= 0)
  {
    if (int rc = resolve_op(c, held[ia], d)) return rc;
    to_fop(d, tail.g.a);
  }
  if (ib >= 0)
  {
    if (int rc = resolve_op(c, held[ib], d)) return rc;
    to_fop(d, tail.g.b);
  }
  tail.kp = ia >= 0 ? child_kind(held[ia]) : CK_INNER;
  tail.kc = ib >= 0 ? child_kind(held[ib]) : (ed->child_is_tip ? CK_TIP : CK_INNER);
  use_tail = true;
  return 0;
}

// one end of an edge or of an insertion candidate in HBM: its tip codes, or its CLV and scaler vector
static int end_in_hbm(pllgpu_ctx *c, unsigned clv, int scaler, bool is_tip, const double *&data, const unsigned char *&codes, const unsigned *&sc)
{
  data = nullptr;
  codes = nullptr;
  if (is_tip)
  {
    if (clv >= c->geo.tips || !c->tipchars[clv].p) return fail(PLLGPU_EINVAL, "tip %u has no codes on the device", clv);
    codes = c->tipchars[clv].p;
  }
  else
  {
    if (!c->clv[clv].p) return fail(PLLGPU_EINVAL, "CLV %u was never computed or uploaded", clv);
    data = c->clv[clv].p;
  }
  return scaler_ptr(c, scaler, sc);
}

// the end P is applied on (an edge's child end, an insertion's subtree end) and the matrix
static int build_edge_child(pllgpu_ctx *c, unsigned clv, int scaler, unsigned matrix, bool is_tip, DevEdge &e)
{
  if (int rc = end_in_hbm(c, clv, scaler, is_tip, e.child, e.ctip, e.cscaler)) return rc;
  e.mat = c->pmat.p + (size_t)matrix * c->pm_stride;
  return 0;
}

// the edge as the kernels read it: its two ends in HBM
static int build_edge(pllgpu_ctx *c, const pllgpu_edge_t *ed, DevEdge &e)
{
  memset(&e, 0, sizeof e);
  if (!c->clv[ed->parent_clv].p) return fail(PLLGPU_EINVAL, "CLV %u was never computed or uploaded", ed->parent_clv);
  e.parent = c->clv[ed->parent_clv].p;
  if (int rc = build_edge_child(c, ed->child_clv, ed->child_scaler, ed->matrix, ed->child_is_tip != 0, e)) return rc;
  if (int rc = scaler_ptr(c, ed->parent_scaler, e.pscaler)) return rc;
  e.layout = (c->clv_aos[ed->parent_clv] ? kAosParent : 0u) | ((!ed->child_is_tip && c->clv_aos[ed->child_clv]) ? kAosLeft : 0u);
  if (e.layout && !ed->gather) return fail(PLLGPU_EINVAL, "a class-compressed CLV met an evaluation without the gather flag");
  if (ed->gather)
  {
    e.psid = c->ids[ed->parent_clv] ? wide_map(c, ed->parent_clv) : nullptr;
    e.csid = c->ids[ed->child_clv] ? wide_map(c, ed->child_clv) : nullptr;
  }
  e.is_root = 0;
  return 0;
}

// the two ends of the edge as chains: the held ones, a chain of no steps around an end that is in HBM
static int build_chain_tail(pllgpu_ctx *c, const pllgpu_edge_t *ed, const DevEdge &e, int held_p, int held_c, ChainTailCall &ct)
{
  const ChainPlan &pl = *c->plan;
  memset(&ct.hp, 0, sizeof ct.hp);
  memset(&ct.hc, 0, sizeof ct.hc);
  const unsigned clv_bytes = (unsigned)(clv_elems(c, pl.entries) * sizeof(double));
  const unsigned sc_bytes = pl.entries * (c->gg.scale_mode == 2 ? 16u : 4u);
  const unsigned any_end = pl.heads[0].first + pl.heads[0].nsteps; // a CS_END step: what a chain of no steps "fetches"
  if (held_p >= 0)
    ct.hp = pl.heads[held_p];
  else
  {
    ct.hp.acc0.data = e.parent;
    ct.hp.acc0.scaler = e.pscaler;
    ct.hp.bacc.clv = clv_bytes;
    ct.hp.bacc.aux = e.pscaler ? sc_bytes : 0u;
    ct.hp.first = any_end;
  }
  if (held_c >= 0)
    ct.hc = pl.heads[held_c];
  else if (ed->child_is_tip)
  {
    ct.hc.acc0.data = e.ctip;
    ct.hc.bacc.aux = (pl.entries + 3u) & ~3u;
    ct.hc.acc_tip = 1u;
    ct.hc.first = any_end;
  }
  else
  {
    ct.hc.acc0.data = e.child;
    ct.hc.acc0.scaler = e.cscaler;
    ct.hc.bacc.clv = clv_bytes;
    ct.hc.bacc.aux = e.cscaler ? sc_bytes : 0u;
    ct.hc.first = any_end;
  }
  const int vp = held_p >= 0 ? (int)pl.head_variant[held_p] : -1, vc = held_c >= 0 ? (int)pl.head_variant[held_c] : -1;
  ct.variant = (unsigned)((vp < 0) ? vc : (vc < 0) ? vp : (vp == vc ? vp : 3));
  ct.in_kernarg = pl.in_kernarg;
  if (!ct.in_kernarg) return 0;
  memset(&ct.pack, 0, sizeof ct.pack);
  unsigned ns = 0;
  ChainHead *hh[2] = {&ct.hp, &ct.hc};
  const int held[2] = {held_p, held_c};
  for (int k = 0; k < 2; ++k)
  {
    const unsigned nst = held[k] >= 0 ? hh[k]->nsteps : 0u;
    if (ns + nst + 1 > (unsigned)kChainPackSteps) return fail(PLLGPU_ERUNTIME, "chain tail does not fit its descriptor pack");
    if (held[k] >= 0)
    {
      memcpy(&ct.pack.loads[ns], &pl.loads[hh[k]->first], (nst + 1) * sizeof(ChainStepLoad));
      memcpy(&ct.pack.ops[ns], &pl.sops[hh[k]->first], (nst + 1) * sizeof(ChainStepOp));
    }
    else
      ct.pack.loads[ns].flags = CS_END;
    hh[k]->first = ns;
    ns += nst + 1;
    ct.pack.heads[k] = *hh[k];
  }
  return 0;
}

extern "C" int pllgpu_edge_loglikelihood(pllgpu_ctx_t *c, const pllgpu_edge_t *ed, double *persite_host, double *lnl_out)
{
  CHECK_CTX_KEEP(c);
  if (int rc = check_edge(c, ed, persite_host)) return rc;
  struct SeqScope
  {
    pllgpu_ctx *c;
    ~SeqScope() { c->seq_override = 0.0; }
  } seq_scope_{c};
  c->seq_override = ed->sequence;
  // an end that the lean tree launch left unstored is stored first; any other edge reads nothing that is pending (the
  // evaluated edge's own matrix, new or not, is no concern of theirs: a cherry that read it kept the old one aside when it
  // changed - matrices_change)
  if (int rc = materialise_if_an_end_is_pending(c, ed, false)) return rc;
  ClaimedWork claimed(c);
  TailCall tail;
  bool use_tail = false;
  int held_p = -1, held_c = -1;
  if (int rc = claim_held_chains(c, ed, claimed, held_p, held_c)) return rc;
  if (int rc = claim_held_ops(c, ed, claimed, tail, use_tail)) return rc;
  DevEdge e;
  if (int rc = build_edge(c, ed, e)) return rc;
  int rc;
  if (held_p >= 0 || held_c >= 0)
  {
    ChainTailCall ct;
    TreePack tp;
    if (claimed.tree)
    {
      tp.end[0] = c->plan->tree_end[held_p];
      tp.end[1] = c->plan->tree_end[held_c];
      ct.tree = &tp;
      ct.lean = c->lazy_cherries;
      ct.deep = ct.lean && c->tree_deep;
    }
    else if (int brc = build_chain_tail(c, ed, e, held_p, held_c, ct))
      return brc;
    rc = run_lnl(c, e, ed->child_is_tip != 0, false, ed->freqs_indices, persite_host, lnl_out, ed->device_result, nullptr, &ct);
    if (rc == 0 && ct.lean)
    {
      // issued: from here on the cherries - or the whole groups - are pending (on a failure ClaimedWork sends the plan out
      // the ordinary way, which stores everything: nothing pending)
      set_pending(c, c->plan, ct.deep);
    }
  }
  else if (use_tail)
  {
    // memory-side descriptors of the ends that were NOT held
    tail.g.p.left = e.parent;
    tail.g.p.lscaler = e.pscaler;
    tail.g.p.right = e.child;
    tail.g.p.rtip = e.ctip;
    tail.g.p.rscaler = e.cscaler;
    rc = run_lnl(c, e, ed->child_is_tip != 0, false, ed->freqs_indices, persite_host, lnl_out, ed->device_result, &tail);
  }
  else
    return run_lnl(c, e, ed->child_is_tip != 0, ed->gather != 0, ed->freqs_indices, persite_host, lnl_out, ed->device_result);
  if (rc == 0) claimed.disarm();
  return rc;
}

extern "C" int pllgpu_root_loglikelihood(pllgpu_ctx_t *c, unsigned clv, int scaler, unsigned gather,
                                         const unsigned *freqs_indices, double *persite_host, double *lnl_out)
{
  CHECK_CTX(c);
  if (clv >= c->geo.nodes || !c->clv[clv].p) return fail(PLLGPU_EINVAL, "CLV %u unavailable on the device", clv);
  DevEdge e;
  memset(&e, 0, sizeof e);
  e.parent = c->clv[clv].p;
  if (int rc = scaler_ptr(c, scaler, e.pscaler)) return rc;
  if (gather) e.psid = c->ids[clv] ? wide_map(c, clv) : nullptr;
  e.layout = c->clv_aos[clv] ? kAosParent : 0u;
  if (e.layout && !gather) return fail(PLLGPU_EINVAL, "a class-compressed CLV met an evaluation without the gather flag");
  e.is_root = 1;
  return run_lnl(c, e, false, gather != 0, freqs_indices, persite_host, lnl_out);
}

// ---- batched insertion log-likelihoods (kernels_insertion.h) -------------------------------------------------
// candidates of one launch: their descriptors must fit one piece of the pinned block, their partial slots stay modest
constexpr unsigned kInsMaxCands = 16384;          // 1 MB of descriptors, well below the grid's y limit
constexpr size_t kInsMaxSlots = (size_t)4 << 20;  // 32 MB of partial sums per launch
constexpr size_t kInsLdsMax = 144 * 1024;         // the inserted node's tile in LDS, beside the kernel's static 8 KB
constexpr size_t kPlcLdsMax = 126 * 1024;         // ... beside k_placement_tiled's static 32 KB (the flags, 7 KB per query of the chunk, the hand-off's words)

// keep (1) or form again in pass 2 (0): do the node tiles a workgroup would park, `bytes` of them, fit the kernel's share of LDS?
static unsigned keep_in_lds(size_t bytes, size_t limit) { return bytes <= limit ? 1u : 0u; }

// Scratch that no kept plan points at: (re)allocating it must not move the context's allocation epoch, or the first
// batched call would drop every cached launch plan of the partition.
struct ScratchEpoch
{
  unsigned long long *prev, none = 0;
  ScratchEpoch() : prev(t_epoch) { t_epoch = &none; }
  ~ScratchEpoch() { t_epoch = prev; }
};

// ---- what every batched call is made of ---------------------------------------------------
// The refusals and checks that need no device state, each with the call's noun in its message. A call runs them and
// its own list checks in its own order: the order decides which error a doubly wrong input reports.
static int refuse_ascertainment(const pllgpu_ctx *c, const char *noun)
{
  if (c->geo.sites == 0 || c->geo.sites != c->geo.sites_alloc) return fail(PLLGPU_EUNSUPPORTED, "%s with ascertainment-bias entries", noun);
  return 0;
}

static int check_rate_indices(const pllgpu_ctx *c, const char *name, const unsigned *indices)
{
  for (unsigned k = 0; k < c->geo.rate_cats; ++k)
    if (indices[k] >= c->geo.rate_matrices) return fail(PLLGPU_EINVAL, "%s[%u] = %u out of range", name, k, indices[k]);
  return 0;
}

static int refuse_compressed(const pllgpu_ctx *c, const char *noun)
{
  for (unsigned n = 0; n < c->geo.nodes; ++n)
    if (c->ids[n] || c->clv_aos[n]) return fail(PLLGPU_EUNSUPPORTED, "%s over class-compressed CLVs", noun);
  return 0;
}

// Last of the preamble, the first step that touches device state: whatever pllgpu_update_partials holds back goes out as
// ordinary launches (an item of the list may name what it produces), then the model of the launches in a zeroed e.
static int batch_edge(pllgpu_ctx *c, DevEdge &e, const unsigned *rate_indices)
{
  if (HOLDS_WORK(c) || !c->pending.empty())
    if (int rc = flush_deferred(c)) return rc;
  memset(&e, 0, sizeof e);
  return fill_edge_model(c, e, rate_indices);
}

// The cutting rule of the one-level calls (include/pll_amd_device.h states it): items per launch, each of `values` sums
// over `blocks` workgroups
static unsigned batch_items(unsigned count, unsigned max_items, unsigned values, unsigned blocks)
{
  return (unsigned)std::min<size_t>(std::min(count, max_items), std::max<size_t>(1, kInsMaxSlots / ((size_t)values * blocks)));
}

// The scratch of a call: `slots` partial sums and `tickets` tickets per launch, `results` values per call, `desc_bytes` of
// descriptors per launch. Tickets are zero between launches; new ones are zeroed here.
static int batch_scratch(pllgpu_ctx *c, DevEdge &e, size_t slots, size_t tickets, size_t results, size_t desc_bytes)
{
  ScratchEpoch scratch_epoch_;
  if (c->ins_partials.ensure(slots) || c->ins_results.ensure(results) || c->ins_cands.ensure(desc_bytes)) return PLLGPU_ENOMEM;
  if (c->ins_tickets.cap < tickets)
  {
    if (c->ins_tickets.ensure(tickets)) return PLLGPU_ENOMEM;
    HIP_TRY(hipMemsetAsync(c->ins_tickets.p, 0, c->ins_tickets.cap * sizeof(unsigned), c->stream));
  }
  e.block_sums = c->ins_partials.p;
  e.counter = c->ins_tickets.p;
  return 0;
}

// n descriptors to device_dst: through the pinned block, or from pageable memory that lives until the copy call has
// returned. fill(T &d, unsigned i) writes the i-th; a status other than 0 ends the upload.
template <class T, class Fill>
static int stage_up(pllgpu_ctx *c, void *device_dst, unsigned n, Fill fill)
{
  const size_t bytes = (size_t)n * sizeof(T);
  unsigned char *dev = nullptr;
  T *host = reinterpret_cast<T *>(stage_take(c, bytes, &dev));
  std::vector<T> pageable;
  if (!host)
  {
    pageable.resize(n);
    host = pageable.data();
  }
  for (unsigned i = 0; i < n; ++i)
    if (int rc = fill(host[i], i)) return rc;
  HIP_TRY(hipMemcpyAsync(device_dst, host, bytes, hipMemcpyHostToDevice, c->stream));
  return 0;
}

// how every launch helper ends
static int launched(pllgpu_ctx *c)
{
  ++c->last_launches;
  HIP_TRY(hipGetLastError());
  return 0;
}

// how every call ends: n values of ins_results to the host in one copy, one wait
static int results_down(pllgpu_ctx *c, double *host, size_t n)
{
  HIP_TRY(copy_down(c, host, c->ins_results.p, n * sizeof(double)));
  if (c->defer_down) HIP_TRY(stream_wait(c));
  return 0;
}

static int check_insertion_end(const pllgpu_ctx *c, unsigned clv, int scaler, unsigned matrix, bool is_tip, const char *what, unsigned i)
{
  const pllgpu_geometry_t &g = c->geo;
  if (clv >= g.nodes || matrix >= g.prob_matrices || scaler >= (int)g.scale_buffers)
    return fail(PLLGPU_EINVAL, "candidate %u: %s references an index out of range", i, what);
  if (is_tip && clv >= g.tips) return fail(PLLGPU_EINVAL, "candidate %u: %s is marked as a tip and is none", i, what);
  return 0;
}

// the candidate list of the insertion and placement calls
static int check_candidates(const pllgpu_ctx *c, const pllgpu_insertion_t *cands, unsigned count)
{
  for (unsigned i = 0; i < count; ++i)
  {
    if (int rc = check_insertion_end(c, cands[i].child1_clv, cands[i].child1_scaler, cands[i].child1_matrix, cands[i].child1_is_tip != 0, "child1", i)) return rc;
    if (int rc = check_insertion_end(c, cands[i].child2_clv, cands[i].child2_scaler, cands[i].child2_matrix, cands[i].child2_is_tip != 0, "child2", i)) return rc;
  }
  return 0;
}

// the descriptors of candidates [first, first + n) on the device: the only place an InsCand is filled
static int upload_candidates(pllgpu_ctx *c, const pllgpu_insertion_t *cands, unsigned first, unsigned n)
{
  return stage_up<InsCand>(c, c->ins_cands.p, n, [&](InsCand &d, unsigned i) {
    const pllgpu_insertion_t &q = cands[first + i];
    if (int rc = end_in_hbm(c, q.child1_clv, q.child1_is_tip ? -1 : q.child1_scaler, q.child1_is_tip != 0, d.left, d.ltip, d.lscaler)) return rc;
    if (int rc = end_in_hbm(c, q.child2_clv, q.child2_is_tip ? -1 : q.child2_scaler, q.child2_is_tip != 0, d.right, d.rtip, d.rscaler)) return rc;
    d.lmat = c->pmat.p + (size_t)q.child1_matrix * c->pm_stride;
    d.rmat = c->pmat.p + (size_t)q.child2_matrix * c->pm_stride;
    return 0;
  });
}

// one launch for candidates [first, first + n): their descriptors up, the kernel of the shape
static int launch_insertions(pllgpu_ctx *c, DevEdge e, const TileWalk &w, const pllgpu_insertion_t *cands, unsigned first, unsigned n, bool stip)
{
  if (int rc = upload_candidates(c, cands, first, n)) return rc;
  const InsCand *dc = reinterpret_cast<const InsCand *>(c->ins_cands.p);
  e.result = c->ins_results.p + first;
  if (c->dna_fast)
    with_bools(stip, false, [&](auto ST, auto) {
      hipLaunchKernelGGL((k_insertion_dna<ST()>), dim3(w.blocks, n), dim3(256), 0, c->stream, e, dc, c->gg.scale_mode, w.tiles_per);
    });
  else
  {
    const unsigned threads = tiled_threads(c);
    const size_t node_bytes = (size_t)c->gg.tile_sz * sizeof(double);
    const unsigned keep = keep_in_lds(node_bytes, kInsLdsMax);
    const size_t lds = keep ? node_bytes : 0;
    const unsigned long long *tm = tipmap_ptr(c);
    with_ich(c->ich, [&](auto ICH) {
      with_bools(stip, false, [&](auto ST, auto) {
        raise_lds_limit(reinterpret_cast<const void *>(&k_insertion_tiled<ICH(), ST()>), c->device, lds);
        hipLaunchKernelGGL((k_insertion_tiled<ICH(), ST()>), dim3(w.blocks, n), dim3(threads), lds, c->stream, e, dc, c->gg, tm, w.tiles_per, keep);
      });
    });
  }
  return launched(c);
}

extern "C" int pllgpu_insertion_loglikelihoods(pllgpu_ctx_t *c, unsigned subtree_clv, int subtree_scaler, unsigned subtree_matrix,
                                               unsigned subtree_is_tip, const pllgpu_insertion_t *cands, unsigned count,
                                               const unsigned *freqs_indices, double *host_out)
{
  CHECK_CTX_KEEP(c);
  const pllgpu_geometry_t &g = c->geo;
  c->last_launches = 0;
  if (!count) return 0;
  static const char noun[] = "insertion log-likelihoods";
  // everything that needs no device state, for the whole list, before held work is touched
  if (!cands || !host_out || !freqs_indices) return fail(PLLGPU_EINVAL, "%s: null argument", noun);
  if (int rc = refuse_ascertainment(c, noun)) return rc;
  if (subtree_clv >= g.nodes || subtree_matrix >= g.prob_matrices || subtree_scaler >= (int)g.scale_buffers || (subtree_is_tip && subtree_clv >= g.tips))
    return fail(PLLGPU_EINVAL, "the subtree end references an index out of range");
  if (int rc = check_rate_indices(c, "freqs_indices", freqs_indices)) return rc;
  if (int rc = check_candidates(c, cands, count)) return rc;
  if (int rc = refuse_compressed(c, noun)) return rc;
  DevEdge e;
  if (int rc = batch_edge(c, e, freqs_indices)) return rc;
  if (int rc = build_edge_child(c, subtree_clv, subtree_is_tip ? -1 : subtree_scaler, subtree_matrix, subtree_is_tip != 0, e)) return rc;

  const TileWalk w = tile_walk(c);
  const unsigned per_launch = batch_items(count, kInsMaxCands, 1, w.blocks);
  if (int rc = batch_scratch(c, e, (size_t)per_launch * w.blocks, per_launch, count, (size_t)per_launch * sizeof(InsCand))) return rc;
  for (unsigned first = 0; first < count; first += per_launch)
    if (int rc = launch_insertions(c, e, w, cands, first, std::min(per_launch, count - first), subtree_is_tip != 0)) return rc;
  return results_down(c, host_out, count);
}

// ---- batched placement log-likelihoods (kernels_placement.h) -------------------------------------------------
// The cutting rule of pllgpu_placement_loglikelihoods (include/pll_amd_device.h states it): candidates per launch, queries
// per launch (whole chunks), the chunk of the shape.
struct PlacementCut
{
  unsigned blocks, tiles_per, chunk, cands, queries;
};

static_assert(kPlcDnaChunk == PLLGPU_PLACEMENT_CHUNK_DNA && kPlcTiledChunk == PLLGPU_PLACEMENT_CHUNK_TILED &&
                  kInsMaxCands == PLLGPU_INSERTION_MAX_CANDS && kInsMaxSlots == PLLGPU_INSERTION_MAX_SLOTS,
              "the cutting rule as include/pll_amd_device.h states it");

static PlacementCut placement_cut(const pllgpu_ctx *c, unsigned queries, unsigned count)
{
  PlacementCut k;
  const TileWalk w = tile_walk(c);
  k.blocks = w.blocks;
  k.tiles_per = w.tiles_per;
  k.chunk = c->dna_fast ? kPlcDnaChunk : kPlcTiledChunk;
  k.cands = batch_items(count, kInsMaxCands, k.chunk, k.blocks); // a candidate with one chunk of queries
  const size_t chunks = std::min<size_t>(std::max<size_t>(1, kInsMaxSlots / ((size_t)k.blocks * k.cands) / k.chunk), 65535u);
  k.queries = (unsigned)std::min<size_t>(queries, chunks * k.chunk);
  return k;
}

// one launch: queries [q0, q0 + nq) of the call x the n candidates whose descriptors stand in ins_cands
static int launch_placements(pllgpu_ctx *c, DevEdge e, const PlacementCut &k, unsigned q0, unsigned nq, unsigned first, unsigned n, unsigned count)
{
  const InsCand *dc = reinterpret_cast<const InsCand *>(c->ins_cands.p);
  const unsigned char *const *rows = reinterpret_cast<const unsigned char *const *>(c->plc_rows.p) + q0;
  e.result = c->ins_results.p + (size_t)q0 * count + first;
  const dim3 grid(k.blocks, n, (nq + k.chunk - 1) / k.chunk);
  if (c->dna_fast)
    hipLaunchKernelGGL((k_placement_dna<kPlcDnaChunk>), grid, dim3(256), 0, c->stream, e, dc, rows, nq, count, c->gg.scale_mode, k.tiles_per);
  else
  {
    const unsigned threads = tiled_threads(c);
    const size_t node_bytes = (size_t)c->gg.tile_sz * sizeof(double);
    const unsigned keep = keep_in_lds(node_bytes, kPlcLdsMax);
    const size_t lds = keep ? node_bytes : 0;
    const unsigned long long *tm = tipmap_ptr(c);
    with_ich(c->ich, [&](auto ICH) {
      raise_lds_limit(reinterpret_cast<const void *>(&k_placement_tiled<ICH(), kPlcTiledChunk>), c->device, lds);
      hipLaunchKernelGGL((k_placement_tiled<ICH(), kPlcTiledChunk>), grid, dim3(threads), lds, c->stream, e, dc, rows, nq, count, c->gg, tm,
                         k.tiles_per, keep);
    });
  }
  return launched(c);
}

extern "C" int pllgpu_placement_loglikelihoods(pllgpu_ctx_t *c, const unsigned *query_tips, unsigned queries, unsigned pendant_matrix,
                                               const pllgpu_insertion_t *cands, unsigned count, const unsigned *freqs_indices, double *host_out)
{
  CHECK_CTX_KEEP(c);
  const pllgpu_geometry_t &g = c->geo;
  c->last_launches = 0;
  if (!queries || !count) return 0;
  static const char noun[] = "placement log-likelihoods";
  // everything that needs no device state, for both lists, before held work is touched
  if (!query_tips || !cands || !host_out || !freqs_indices) return fail(PLLGPU_EINVAL, "%s: null argument", noun);
  // one query is what the insertion call serves, with the same checks and the same bits: there is no node to share
  if (queries == 1 && query_tips[0] < g.tips)
    return pllgpu_insertion_loglikelihoods(c, query_tips[0], -1, pendant_matrix, 1u, cands, count, freqs_indices, host_out);
  if (int rc = refuse_ascertainment(c, noun)) return rc;
  for (unsigned q = 0; q < queries; ++q)
    if (query_tips[q] >= g.tips) return fail(PLLGPU_EINVAL, "query %u: %u is no tip", q, query_tips[q]);
  if (pendant_matrix >= g.prob_matrices) return fail(PLLGPU_EINVAL, "the pendant matrix index is out of range");
  if (int rc = check_rate_indices(c, "freqs_indices", freqs_indices)) return rc;
  if (int rc = check_candidates(c, cands, count)) return rc;
  if (int rc = refuse_compressed(c, noun)) return rc;
  for (unsigned q = 0; q < queries; ++q)
    if (!c->tipchars[query_tips[q]].p) return fail(PLLGPU_EINVAL, "query %u: tip %u has no codes on the device", q, query_tips[q]);
  DevEdge e;
  if (int rc = batch_edge(c, e, freqs_indices)) return rc;
  e.mat = c->pmat.p + (size_t)pendant_matrix * c->pm_stride;

  const PlacementCut k = placement_cut(c, queries, count);
  const size_t pairs = (size_t)k.queries * k.cands;
  if (int rc = batch_scratch(c, e, pairs * k.blocks, pairs, (size_t)queries * count, (size_t)k.cands * sizeof(InsCand))) return rc;
  {
    ScratchEpoch scratch_epoch_;
    if (c->plc_rows.ensure((size_t)queries * sizeof(const unsigned char *))) return PLLGPU_ENOMEM;
  }
  if (int rc = stage_up<const unsigned char *>(c, c->plc_rows.p, queries, [&](const unsigned char *&row, unsigned q) {
        row = c->tipchars[query_tips[q]].p;
        return 0;
      }))
    return rc;
  for (unsigned first = 0; first < count; first += k.cands)
  {
    const unsigned n = std::min(k.cands, count - first);
    if (int rc = upload_candidates(c, cands, first, n)) return rc;
    for (unsigned q0 = 0; q0 < queries; q0 += k.queries)
      if (int rc = launch_placements(c, e, k, q0, std::min(k.queries, queries - q0), first, n, count)) return rc;
  }
  return results_down(c, host_out, (size_t)queries * count);
}

// ---- batched NNI scores (kernels_quartet.h) ------------------------------------------------------------------
// The cutting rule of pllgpu_quartet_loglikelihoods (include/pll_amd_device.h states it)
constexpr unsigned kQuartetMax = 8192; // 1.1 MB of descriptors: one piece of the pinned block
static_assert(kQuartetMax == PLLGPU_QUARTET_MAX && kQuartetMax * sizeof(QuartetDesc) <= kRingMax, "include/pll_amd_device.h states the cutting rule");

// one launch for quartets [first, first + n): their descriptors up, the kernel of the shape
// (sites: the PS instantiations, which leave every site's value through ps as well)
static int launch_quartets(pllgpu_ctx *c, DevEdge e, const TileWalk &w, const pllgpu_quartet_t *quartets, unsigned first, unsigned n, unsigned count,
                           bool sites = false, const QuartetSites ps = QuartetSites{nullptr, nullptr})
{
  const int up = stage_up<QuartetDesc>(c, c->ins_cands.p, n, [&](QuartetDesc &d, unsigned i) {
    const pllgpu_quartet_t &q = quartets[first + i];
    d.tt_rule = 0u;
    d.pad_ = 0u;
    for (unsigned x = 0; x < 4; ++x)
    {
      const bool tip = (q.is_tip[x] & PLLGPU_QUARTET_TIP_CODES) != 0;
      if (int rc = end_in_hbm(c, q.clv[x], tip ? -1 : q.scaler[x], tip, d.end[x].clv, d.end[x].tip, d.end[x].scaler)) return rc;
      d.end[x].mat = c->pmat.p + (size_t)q.matrix[x] * c->pm_stride;
      if (tip && (q.is_tip[x] & PLLGPU_QUARTET_TIP_PATTERN)) d.tt_rule |= 1u << x;
    }
    d.inner = c->pmat.p + (size_t)q.inner_matrix * c->pm_stride;
    return 0;
  });
  if (up) return up;
  const QuartetDesc *dq = reinterpret_cast<const QuartetDesc *>(c->ins_cands.p);
  e.result = c->ins_results.p + first; // [arrangement][quartet of the call]
  if (c->dna_fast)
    with_bools(sites, false, [&](auto PS, auto) {
      if (c->gg.scale_mode == 2)
        hipLaunchKernelGGL((k_quartet_dna<2, PS()>), dim3(w.blocks, n), dim3(256), 0, c->stream, e, dq, count, w.tiles_per, ps);
      else
        hipLaunchKernelGGL((k_quartet_dna<1, PS()>), dim3(w.blocks, n), dim3(256), 0, c->stream, e, dq, count, w.tiles_per, ps);
    });
  else
  {
    const size_t node_bytes = (size_t)c->gg.R * c->gg.S * 64u * sizeof(double);
    // both nodes of an arrangement in LDS, or (recompute path) one rate of the second node per wave
    const unsigned keep = keep_in_lds(2 * node_bytes, kInsLdsMax);
    const size_t lds = keep ? 2 * node_bytes : (size_t)tiled_waves(c) * c->gg.S * 64u * sizeof(double);
    const unsigned long long *tm = tipmap_ptr(c);
    with_ich(c->ich, [&](auto ICH) {
      with_bools(sites, false, [&](auto PS, auto) {
        raise_lds_limit(reinterpret_cast<const void *>(&k_quartet_tiled<ICH(), PS()>), c->device, lds);
        hipLaunchKernelGGL((k_quartet_tiled<ICH(), PS()>), dim3(w.blocks, n), dim3(tiled_threads(c)), lds, c->stream, e, dq, c->gg, tm, count, w.tiles_per, keep, ps);
      });
    });
  }
  return launched(c);
}

// What the quartet calls do before anything is allocated: everything that needs no device state, for the whole list,
// before held work is touched; held work out; the model of the launches in e.
static int quartet_call_begin(pllgpu_ctx *c, const pllgpu_quartet_t *quartets, unsigned count, const unsigned *freqs_indices, DevEdge &e)
{
  static const char noun[] = "quartet log-likelihoods";
  const pllgpu_geometry_t &g = c->geo;
  if (int rc = refuse_ascertainment(c, noun)) return rc;
  if (int rc = check_rate_indices(c, "freqs_indices", freqs_indices)) return rc;
  for (unsigned i = 0; i < count; ++i)
  {
    const pllgpu_quartet_t &q = quartets[i];
    for (unsigned x = 0; x < 4; ++x)
    {
      if (q.clv[x] >= g.nodes || q.matrix[x] >= g.prob_matrices || q.scaler[x] >= (int)g.scale_buffers)
        return fail(PLLGPU_EINVAL, "quartet %u: end %u references an index out of range", i, x);
      if (q.is_tip[x] && (!(q.is_tip[x] & PLLGPU_QUARTET_TIP_CODES) || q.clv[x] >= g.tips))
        return fail(PLLGPU_EINVAL, "quartet %u: end %u is marked as a tip and is none", i, x);
    }
    if (q.inner_matrix >= g.prob_matrices) return fail(PLLGPU_EINVAL, "quartet %u: the inner matrix index is out of range", i);
  }
  if (int rc = refuse_compressed(c, noun)) return rc;
  return batch_edge(c, e, freqs_indices);
}

// slots, tickets, results and descriptors of launches of up to per_launch quartets of a call of `count`
static int quartet_scratch(pllgpu_ctx *c, DevEdge &e, unsigned per_launch, unsigned blocks, unsigned count)
{
  return batch_scratch(c, e, (size_t)3 * per_launch * blocks, (size_t)3 * per_launch, (size_t)3 * count, (size_t)per_launch * sizeof(QuartetDesc));
}

// one copy back for all values, one wait; the kernels leave [arrangement][quartet], the caller gets [quartet][3]
static int quartet_sums_down(pllgpu_ctx *c, unsigned count, double *host_out)
{
  std::vector<double> rows((size_t)3 * count);
  if (int rc = results_down(c, rows.data(), rows.size())) return rc;
  for (unsigned i = 0; i < count; ++i)
    for (unsigned a = 0; a < 3; ++a) host_out[(size_t)3 * i + a] = rows[(size_t)a * count + i];
  return 0;
}

extern "C" int pllgpu_quartet_loglikelihoods(pllgpu_ctx_t *c, const pllgpu_quartet_t *quartets, unsigned count, const unsigned *freqs_indices,
                                             double *host_out)
{
  CHECK_CTX_KEEP(c);
  c->last_launches = 0;
  if (!count) return 0;
  if (!quartets || !host_out || !freqs_indices) return fail(PLLGPU_EINVAL, "quartet log-likelihoods: null argument");
  DevEdge e;
  if (int rc = quartet_call_begin(c, quartets, count, freqs_indices, e)) return rc;
  const TileWalk w = tile_walk(c);
  const unsigned per_launch = batch_items(count, kQuartetMax, 3, w.blocks);
  if (int rc = quartet_scratch(c, e, per_launch, w.blocks, count)) return rc;
  for (unsigned first = 0; first < count; first += per_launch)
    if (int rc = launch_quartets(c, e, w, quartets, first, std::min(per_launch, count - first), count)) return rc;
  return quartet_sums_down(c, count, host_out);
}

// ---- resampled quartet log-likelihoods (kernels_resample.h) ---------------------------------
// The cutting rule of pllgpu_quartet_resampled_loglikelihoods (include/pll_amd_device.h states it)
struct ResampleCut
{
  unsigned upad, wstride, splits, split_len;
  unsigned quartets, replicates; // per chunk
};

static ResampleCut resample_cut(unsigned sites, unsigned count, unsigned replicates, bool persite, unsigned per_launch, size_t budget)
{
  ResampleCut k;
  k.upad = (sites + 63u) / 64u * 64u;
  k.wstride = (sites + 3u) / 4u * 4u;
  k.splits = resample_splits(sites);
  k.split_len = resample_split_len(sites);
  // quartets first: their per-site rows may take half of the scratch ...
  const size_t per_quartet = (size_t)3 * sizeof(double) * ((replicates ? k.upad : 0u) + (persite ? sites : 0u));
  k.quartets = (unsigned)std::min<size_t>(std::min(count, per_launch), std::max<size_t>(1, per_quartet ? budget / 2 / per_quartet : count));
  // ... then replicates: a row of weights, its partials and its results take what is left
  const size_t used = per_quartet * k.quartets, left = budget > used ? budget - used : 0;
  const size_t per_replicate = (size_t)k.wstride * sizeof(unsigned) + (size_t)3 * k.quartets * sizeof(double) * (k.splits + 1u);
  k.replicates = (unsigned)std::min<size_t>(replicates, std::max<size_t>(1, left / per_replicate));
  return k;
}

static int resample_events(pllgpu_ctx *c)
{
  for (hipEvent_t &ev : c->rs_ev)
    if (!ev) HIP_TRY(hipEventCreate(&ev));
  return 0;
}

// ---- replicate weights drawn on the device (kernels_rell.h) ----------------------------------
// the prefix sums of the pattern weights the context holds: formed again when the weights have been uploaded since the last
// time, kept otherwise; {total, sites of weight != 1} come back once per rebuild
static int rell_cdf_current(pllgpu_ctx *c)
{
  if (!c->rell) c->rell = new RellState;
  RellState &r = *c->rell;
  if (!r.stale) return 0;
  const unsigned sites = c->geo.sites;
  {
    ScratchEpoch scratch_epoch_;
    if (int rc = r.cdf.ensure((size_t)sites + 2u)) return rc;
  }
  hipLaunchKernelGGL(k_rell_cdf, dim3(1), dim3(256), 0, c->stream, c->pattern_weights.p, r.cdf.p, r.cdf.p + sites, sites);
  if (int rc = launched(c)) return rc;
  unsigned long long summary[2] = {0, 0};
  HIP_TRY(copy_down(c, summary, r.cdf.p + sites, sizeof summary));
  if (c->defer_down) HIP_TRY(stream_wait(c));
  r.total = summary[0];
  r.not_one = summary[1];
  r.stale = false;
  return 0;
}

// (after rell_cdf_current) a row's words are 32 bits, and a replicate of no draws is none
static int rell_check_total(const pllgpu_ctx *c, const char *who)
{
  if (c->rell->total == 0 || (c->rell->total >> 32))
    return fail(PLLGPU_EINVAL, "%s: the pattern weights add up to %llu, a replicate needs a sum in [1, 2^32)", who, c->rell->total);
  return 0;
}

// rows [first, first + nr) of the definition into c->rs_w, wstride words apart: one launch, grid (rows, ranges)
static int launch_rell_draw(pllgpu_ctx *c, unsigned long long seed, unsigned first, unsigned nr, unsigned wstride)
{
  const unsigned sites = c->geo.sites;
  // (a grid's second dimension ends at 65535: only a range lowered for tests on a very long alignment could pass it)
  const unsigned range = std::max(c->rell_range, (sites / 65535u + 4u) / 4u * 4u);
  const unsigned ranges = (sites + range - 1u) / range;
  const size_t lds = (size_t)std::min(range, wstride) * sizeof(unsigned);
  const RellGeo g{seed, first, (unsigned)c->rell->total, sites, wstride, range};
  auto launch = [&](auto kernel) {
    raise_lds_limit(reinterpret_cast<const void *>(kernel), c->device, lds);
    hipLaunchKernelGGL(kernel, dim3(nr, ranges), dim3(kRellThreads), lds, c->stream, c->rell->cdf.p, c->rs_w.p, g);
  };
  if (c->rell->not_one == 0) launch(&k_rell_draw<true>); // every weight is 1: cdf[n] = n + 1, the site is r itself
  else launch(&k_rell_draw<false>);
  return launched(c);
}

// nr rows of c->rs_w to the caller's [nr][sites]: one copy, one wait
static int rell_rows_down(pllgpu_ctx *c, unsigned *host, unsigned nr, unsigned wstride)
{
  const unsigned sites = c->geo.sites;
  if (wstride == sites)
  {
    HIP_TRY(copy_down(c, host, c->rs_w.p, (size_t)nr * sites * sizeof(unsigned)));
    if (c->defer_down) HIP_TRY(stream_wait(c));
    return 0;
  }
  HIP_TRY(hipMemcpy2DAsync(host, (size_t)sites * sizeof(unsigned), c->rs_w.p, (size_t)wstride * sizeof(unsigned), (size_t)sites * sizeof(unsigned), nr,
                           hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(stream_wait(c));
  return 0;
}

// what puts a chunk's rows of weights into c->rs_w: the caller's array, or one k_rell_draw launch for the absolute rows
// r0 .. r0 + nr of `seed` (weights == nullptr), which then go back to weights_out if that is given
struct ResampleRows
{
  const unsigned *weights;
  unsigned long long seed;
  unsigned *weights_out;
};

// both resampling calls after their own argument checks: the quartet checks, the cut, the loop over the chunks, the copies back
static int resampled_run(pllgpu_ctx *c, const pllgpu_quartet_t *quartets, unsigned count, const unsigned *freqs_indices, const ResampleRows &rows,
                         unsigned replicates, double *host_lnl, double *host_resampled, double *host_persite)
{
  const unsigned sites = c->geo.sites;
  const unsigned *weights = rows.weights;
  DevEdge e;
  if (int rc = quartet_call_begin(c, quartets, count, freqs_indices, e)) return rc;
  const TileWalk w = tile_walk(c);
  if (!weights && replicates)
  {
    if (int rc = rell_cdf_current(c)) return rc;
    if (int rc = rell_check_total(c, "rell quartet log-likelihoods")) return rc;
  }

  const ResampleCut k = resample_cut(sites, count, replicates, host_persite != nullptr, batch_items(count, kQuartetMax, 3, w.blocks), c->resample_bytes);
  const bool one_quartet_chunk = k.quartets >= count;
  if (int rc = quartet_scratch(c, e, k.quartets, w.blocks, count)) return rc;
  {
    ScratchEpoch scratch_epoch_;
    if ((replicates && (c->rs_u.ensure((size_t)3 * k.quartets * k.upad) || c->rs_w.ensure((size_t)k.replicates * k.wstride) ||
                        c->rs_part.ensure((size_t)k.splits * 3 * k.quartets * k.replicates) || c->rs_out.ensure((size_t)3 * k.quartets * k.replicates))) ||
        (host_persite && c->rs_weighted.ensure((size_t)3 * k.quartets * sites)))
      return PLLGPU_ENOMEM;
  }
  if (int rc = resample_events(c)) return rc;
  // the small outputs are collected here and handed over once everything has succeeded
  std::vector<double> resampled((size_t)count * replicates * 3), piece((size_t)3 * k.quartets * k.replicates);

  // Replicate chunks outermost: every row of weights goes up once per call. Stage 1 runs once per quartet chunk when the
  // quartets are one chunk (its rows then stay for every replicate chunk), and again per replicate chunk otherwise - the
  // same launch, the same bits.
  for (unsigned r0 = 0; r0 == 0 || r0 < replicates; r0 += std::max(k.replicates, 1u))
  {
    const unsigned nr = replicates ? std::min(k.replicates, replicates - r0) : 0u;
    const bool timed = r0 == 0;
    if (timed) HIP_TRY(hipEventRecord(c->rs_ev[0], c->stream));
    if (nr && !weights)
    {
      if (int rc = launch_rell_draw(c, rows.seed, r0, nr, k.wstride)) return rc;
    }
    else if (nr)
    {
      const unsigned *src = weights + (size_t)r0 * sites;
      if (k.wstride == sites)
        HIP_TRY(hipMemcpyAsync(c->rs_w.p, src, (size_t)nr * sites * sizeof(unsigned), hipMemcpyHostToDevice, c->stream));
      else // rows 16 bytes aligned on the device; what lies between a row's end and the next row is never read
        HIP_TRY(hipMemcpy2DAsync(c->rs_w.p, (size_t)k.wstride * sizeof(unsigned), src, (size_t)sites * sizeof(unsigned), (size_t)sites * sizeof(unsigned),
                                 nr, hipMemcpyHostToDevice, c->stream));
    }
    if (timed) HIP_TRY(hipEventRecord(c->rs_ev[1], c->stream));
    if (nr && rows.weights_out) // one copy back per replicate chunk
      if (int rc = rell_rows_down(c, rows.weights_out + (size_t)r0 * sites, nr, k.wstride)) return rc;
    for (unsigned first = 0; first < count; first += k.quartets)
    {
      const unsigned nq = std::min(k.quartets, count - first);
      const bool want_weighted = host_persite && r0 == 0;
      if (r0 == 0 || !one_quartet_chunk)
      {
        const QuartetSites ps{replicates ? c->rs_u.p : nullptr, want_weighted ? c->rs_weighted.p : nullptr};
        if (int rc = launch_quartets(c, e, w, quartets, first, nq, count, true, ps)) return rc;
      }
      if (timed && first == 0) HIP_TRY(hipEventRecord(c->rs_ev[2], c->stream));
      if (nr)
      {
        const ResampleGeo rg{3u * nq, nr, sites, k.upad, k.wstride, k.split_len};
        hipLaunchKernelGGL(k_resample_mfma, dim3((nr + 127u) / 128u, (rg.V + 31u) / 32u, k.splits), dim3(256), 0, c->stream, c->rs_u.p, c->rs_w.p,
                           c->rs_part.p, rg);
        const size_t total = (size_t)rg.V * nr;
        hipLaunchKernelGGL(k_resample_reduce, dim3((unsigned)((total + 255u) / 256u)), dim3(256), 0, c->stream, c->rs_part.p, c->rs_out.p, rg.V, nr,
                           k.splits);
        c->last_launches += 2;
        HIP_TRY(hipGetLastError());
      }
      if (timed && first == 0) HIP_TRY(hipEventRecord(c->rs_ev[3], c->stream));
      // one copy back per chunk: the weighted per-site rows straight into the caller's array, the sums into `resampled`
      if (want_weighted)
        HIP_TRY(copy_down(c, host_persite + (size_t)3 * first * sites, c->rs_weighted.p, (size_t)3 * nq * sites * sizeof(double)));
      if (nr)
      {
        HIP_TRY(copy_down(c, piece.data(), c->rs_out.p, (size_t)3 * nq * nr * sizeof(double)));
        if (c->defer_down) HIP_TRY(stream_wait(c));
        for (unsigned i = 0; i < nq; ++i)
          for (unsigned a = 0; a < 3; ++a)
            for (unsigned b = 0; b < nr; ++b) resampled[((size_t)(first + i) * replicates + r0 + b) * 3 + a] = piece[((size_t)3 * i + a) * nr + b];
      }
    }
  }
  std::vector<double> lnl((size_t)3 * count);
  if (int rc = quartet_sums_down(c, count, lnl.data())) return rc;
  for (int t = 0; t < 3; ++t)
  {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->rs_ev[t], c->rs_ev[t + 1]));
    c->rs_ms[t] = (double)ms;
  }
  if (host_lnl) memcpy(host_lnl, lnl.data(), lnl.size() * sizeof(double));
  if (replicates) memcpy(host_resampled, resampled.data(), resampled.size() * sizeof(double));
  return 0;
}

extern "C" int pllgpu_quartet_resampled_loglikelihoods(pllgpu_ctx_t *c, const pllgpu_quartet_t *quartets, unsigned count, const unsigned *freqs_indices,
                                                       const unsigned *weights, unsigned replicates, double *host_lnl, double *host_resampled,
                                                       double *host_persite)
{
  CHECK_CTX_KEEP(c);
  c->last_launches = 0;
  if (!count) return 0;
  if (!quartets || !freqs_indices) return fail(PLLGPU_EINVAL, "resampled quartet log-likelihoods: null argument");
  if (replicates && (!weights || !host_resampled)) return fail(PLLGPU_EINVAL, "resampled quartet log-likelihoods: replicates without weights or results");
  if (!host_lnl && !host_resampled && !host_persite) return fail(PLLGPU_EINVAL, "resampled quartet log-likelihoods: no output asked for");
  return resampled_run(c, quartets, count, freqs_indices, ResampleRows{weights, 0ull, nullptr}, replicates, host_lnl, host_resampled, host_persite);
}

extern "C" int pllgpu_quartet_rell_loglikelihoods(pllgpu_ctx_t *c, const pllgpu_quartet_t *quartets, unsigned count, const unsigned *freqs_indices,
                                                  unsigned long long seed, unsigned replicates, double *host_lnl, double *host_resampled,
                                                  double *host_persite, unsigned *host_weights_out)
{
  CHECK_CTX_KEEP(c);
  c->last_launches = 0;
  if (!count) return 0;
  if (!quartets || !freqs_indices) return fail(PLLGPU_EINVAL, "rell quartet log-likelihoods: null argument");
  if (replicates && !host_resampled) return fail(PLLGPU_EINVAL, "rell quartet log-likelihoods: replicates without results");
  if (!host_lnl && !host_resampled && !host_persite) return fail(PLLGPU_EINVAL, "rell quartet log-likelihoods: no output asked for");
  return resampled_run(c, quartets, count, freqs_indices, ResampleRows{nullptr, seed, host_weights_out}, replicates, host_lnl, host_resampled,
                       host_persite);
}

extern "C" int pllgpu_replicate_weights_draw(pllgpu_ctx_t *c, unsigned long long seed, unsigned first, unsigned replicates, unsigned *host_out)
{
  CHECK_CTX_KEEP(c); // (no CLV is read: held work stays held)
  const pllgpu_geometry_t &g = c->geo;
  c->last_launches = 0;
  if (!replicates) return 0;
  static const char noun[] = "replicate weights";
  if (!host_out) return fail(PLLGPU_EINVAL, "%s: null argument", noun);
  // rows that the quartet call could not take are not handed out: its refusals, with its status
  if (int rc = refuse_ascertainment(c, noun)) return rc;
  if (int rc = refuse_compressed(c, noun)) return rc;
  if (int rc = rell_cdf_current(c)) return rc;
  if (int rc = rell_check_total(c, noun)) return rc;
  const unsigned wstride = (g.sites + 3u) / 4u * 4u;
  const unsigned per_chunk = (unsigned)std::min<size_t>(replicates, std::max<size_t>(1, c->resample_bytes / ((size_t)wstride * sizeof(unsigned))));
  {
    ScratchEpoch scratch_epoch_;
    if (int rc = c->rs_w.ensure((size_t)per_chunk * wstride)) return rc;
  }
  for (unsigned r0 = 0; r0 < replicates; r0 += per_chunk)
  {
    const unsigned nr = std::min(per_chunk, replicates - r0);
    if (int rc = launch_rell_draw(c, seed, first + r0, nr, wstride)) return rc;
    if (int rc = rell_rows_down(c, host_out + (size_t)r0 * g.sites, nr, wstride)) return rc;
  }
  return 0;
}

extern "C" int pllgpu_resample_last_times(const pllgpu_ctx_t *c, double *ms)
{
  if (!c || !ms) return fail(PLLGPU_EINVAL, "null argument");
  for (int t = 0; t < 3; ++t) ms[t] = c->rs_ms[t];
  return 0;
}

// ---- the branch-length gradient (kernels_gradient.h) -------------------------------------------------------------
// The cutting rule of pllgpu_branch_derivatives (include/pll_amd_device.h states it)
constexpr unsigned kBranchMax = 8192; // 512 KB of descriptors: one piece of the pinned block
static_assert(kBranchMax == PLLGPU_BRANCH_MAX && kBranchMax * sizeof(BranchDesc) <= kRingMax, "include/pll_amd_device.h states the cutting rule");
constexpr size_t kGradLdsMax = 152 * 1024; // k_gradient_tiled's dynamic LDS, beside its static 8 KB

// the dynamic LDS of k_gradient_tiled: the branch's diag table [R][S][4]; cat: and the two [R][64] rows of the categories
static size_t branch_lds(const pllgpu_ctx *c, bool cat)
{
  return ((size_t)c->gg.R * c->gg.S * 4 + (cat ? (size_t)2 * c->gg.R * 64 : 0)) * sizeof(double);
}

// the descriptor of one branch of a list (every call over pllgpu_branch_t rows)
static int branch_desc(pllgpu_ctx *c, const pllgpu_branch_t &q, BranchDesc &d)
{
  // an end given by codes takes the left role, as in pllgpu_update_sumtable's callers; otherwise parent left, child right
  const bool swap = q.child_is_tip != 0;
  const unsigned lclv = swap ? q.child_clv : q.parent_clv, rclv = swap ? q.parent_clv : q.child_clv;
  const int lsc = swap ? q.child_scaler : q.parent_scaler, rsc = swap ? q.parent_scaler : q.child_scaler;
  const bool ltip = (swap ? q.child_is_tip : q.parent_is_tip) != 0;
  // per-site counts cancel in L'/L: only the per-rate form is read
  const bool counts = c->geo.per_rate_scalers != 0;
  if (int rc = end_in_hbm(c, lclv, (ltip || !counts) ? -1 : lsc, ltip, d.left, d.ltip, d.lscaler)) return rc;
  if (int rc = end_in_hbm(c, rclv, counts ? rsc : -1, false, d.right, d.rtip, d.rscaler)) return rc;
  d.t = q.branch_length;
  d.pad_ = 0.0;
  return 0;
}

// one launch for branches [first, first + n): their descriptors up, the kernel of the shape. cat: the R + 2 values of
// pllgpu_branch_category_derivatives instead of the two of pllgpu_branch_derivatives
static int launch_branches(pllgpu_ctx *c, DevEdge e, const TileWalk &w, const DevDiag &dg, const pllgpu_branch_t *branches, unsigned first, unsigned n,
                           unsigned count, bool cat)
{
  const int up = stage_up<BranchDesc>(c, c->ins_cands.p, n, [&](BranchDesc &d, unsigned i) { return branch_desc(c, branches[first + i], d); });
  if (up) return up;
  const BranchDesc *db = reinterpret_cast<const BranchDesc *>(c->ins_cands.p);
  const double *m1 = c->pmat.p + (size_t)c->geo.prob_matrices * c->pm_stride, *m2 = m1 + c->pm_stride;
  e.result = c->ins_results.p + first; // [d_f | dd_f | d_cat[0..R)][branch of the call]
  if (c->dna_fast)
    with_bools(cat, false, [&](auto CAT, auto) {
      hipLaunchKernelGGL(k_gradient_dna<CAT()>, dim3(w.blocks, n), dim3(256), 0, c->stream, e, dg, db, m1, m2, count, w.tiles_per);
    });
  else
  {
    const size_t lds = branch_lds(c, cat);
    const unsigned long long *tm = tipmap_ptr(c);
    with_ich(c->ich, [&](auto ICH) {
      with_bools(cat, false, [&](auto CAT, auto) {
        raise_lds_limit(reinterpret_cast<const void *>(&k_gradient_tiled<ICH(), CAT()>), c->device, lds);
        hipLaunchKernelGGL((k_gradient_tiled<ICH(), CAT()>), dim3(w.blocks, n), dim3(tiled_threads(c)), lds, c->stream, e, dg, db, m1, m2, c->gg, tm, count,
                           w.tiles_per);
      });
    });
  }
  return launched(c);
}

// What both gradient entries do after their own argument checks, in the order include/pll_amd_device.h states: the list
// checks and refusals that need no device state, then - the first step that touches it - held work out, the model of the
// launches in e and the branch's model in dg. outputs_ok: the entry's own outputs are there.
static int branch_call_begin(pllgpu_ctx *c, const pllgpu_branch_t *branches, unsigned count, const unsigned *params_indices, bool outputs_ok,
                             const char *noun, DevEdge &e, DevDiag &dg)
{
  const pllgpu_geometry_t &g = c->geo;
  // everything that needs no device state, for the whole list, before held work is touched
  if (!branches || !outputs_ok || !params_indices) return fail(PLLGPU_EINVAL, "%s: null argument", noun);
  if (int rc = refuse_ascertainment(c, noun)) return rc;
  if (int rc = check_rate_indices(c, "params_indices", params_indices)) return rc;
  for (unsigned i = 0; i < count; ++i)
  {
    const pllgpu_branch_t &q = branches[i];
    if (q.parent_clv >= g.nodes || q.child_clv >= g.nodes || q.parent_scaler >= (int)g.scale_buffers || q.child_scaler >= (int)g.scale_buffers)
      return fail(PLLGPU_EINVAL, "branch %u references an index out of range", i);
    if ((q.parent_is_tip && q.parent_clv >= g.tips) || (q.child_is_tip && q.child_clv >= g.tips))
      return fail(PLLGPU_EINVAL, "branch %u: an end is marked as a tip and is none", i);
    if (q.parent_is_tip && q.child_is_tip) return fail(PLLGPU_EINVAL, "branch %u: both ends are given by codes", i);
    if (!(q.branch_length >= 0.0) || !std::isfinite(q.branch_length)) return fail(PLLGPU_EINVAL, "branch %u: the length is negative or not finite", i);
  }
  if (int rc = refuse_compressed(c, noun)) return rc;
  if (!c->eigenvals.p || !c->rates.p) return fail(PLLGPU_EINVAL, "eigenvalues / category rates were not uploaded");
  if (int rc = batch_edge(c, e, params_indices)) return rc;
  memset(&dg, 0, sizeof dg);
  for (unsigned k = 0; k < g.rate_cats; ++k) dg.fidx[k] = (unsigned char)params_indices[k];
  dg.eigenvals = c->eigenvals.p;
  dg.rates = c->rates.p;
  dg.prop_invar = c->prop_invar.p;
  dg.S = g.states;
  dg.SP = g.states_padded;
  dg.R = g.rate_cats;
  return 0;
}

extern "C" int pllgpu_branch_derivatives(pllgpu_ctx_t *c, const pllgpu_branch_t *branches, unsigned count, const unsigned *params_indices,
                                         double *host_d, double *host_dd)
{
  CHECK_CTX_KEEP(c);
  c->last_launches = 0;
  if (!count) return 0;
  DevEdge e;
  DevDiag dg;
  if (int rc = branch_call_begin(c, branches, count, params_indices, host_d != nullptr, "branch derivatives", e, dg)) return rc;

  const TileWalk w = tile_walk(c);
  const unsigned per_launch = batch_items(count, kBranchMax, 2, w.blocks);
  if (int rc = batch_scratch(c, e, (size_t)2 * per_launch * w.blocks, (size_t)2 * per_launch, (size_t)2 * count, (size_t)per_launch * sizeof(BranchDesc)))
    return rc;
  for (unsigned first = 0; first < count; first += per_launch)
    if (int rc = launch_branches(c, e, w, dg, branches, first, std::min(per_launch, count - first), count, false)) return rc;
  // the kernels leave [d_f | dd_f][branch]
  std::vector<double> rows((size_t)2 * count);
  if (int rc = results_down(c, rows.data(), rows.size())) return rc;
  memcpy(host_d, rows.data(), (size_t)count * sizeof(double));
  if (host_dd) memcpy(host_dd, rows.data() + count, (size_t)count * sizeof(double));
  return 0;
}

// The per-category form (include/pll_amd_device.h states its cutting rule): R + 2 values per branch, then - when the
// contraction is asked for - the lengths of the whole list up once and k_rate_gradient behind the last cut.
extern "C" int pllgpu_branch_category_derivatives(pllgpu_ctx_t *c, const pllgpu_branch_t *branches, unsigned count, const unsigned *params_indices,
                                                  double *host_d_cat, double *host_d, double *host_dd, double *host_d_rates, double *host_d_scale)
{
  CHECK_CTX_KEEP(c);
  const unsigned R = c->geo.rate_cats, V = R + 2u;
  c->last_launches = 0;
  const bool want_sums = host_d_rates || host_d_scale;
  if (!count)
  {
    // sums over no branch
    if (host_d_rates) std::fill(host_d_rates, host_d_rates + R, 0.0);
    if (host_d_scale) *host_d_scale = 0.0;
    return 0;
  }
  static const char noun[] = "branch category derivatives";
  if (!host_d_cat && !host_d && !host_dd && !want_sums) return fail(PLLGPU_EINVAL, "%s: no output asked for", noun);
  DevEdge e;
  DevDiag dg;
  if (int rc = branch_call_begin(c, branches, count, params_indices, true, noun, e, dg)) return rc;
  if (!c->dna_fast && branch_lds(c, true) > kGradLdsMax)
    return fail(PLLGPU_EUNSUPPORTED, "%s: %u states x %u rate categories need %zu bytes of LDS per workgroup", noun, c->geo.states, R, branch_lds(c, true));

  const TileWalk w = tile_walk(c);
  const unsigned per_launch = batch_items(count, kBranchMax, V, w.blocks);
  // results: [R + 2][count] from the kernels, then the lengths [count] and k_rate_gradient's [R + 1]
  const size_t values = (size_t)V * count, tail = want_sums ? (size_t)count + R + 1u : 0u;
  if (int rc = batch_scratch(c, e, (size_t)V * per_launch * w.blocks, (size_t)V * per_launch, values + tail, (size_t)per_launch * sizeof(BranchDesc)))
    return rc;
  for (unsigned first = 0; first < count; first += per_launch)
    if (int rc = launch_branches(c, e, w, dg, branches, first, std::min(per_launch, count - first), count, true)) return rc;
  if (want_sums)
  {
    double *lengths = c->ins_results.p + values, *out = lengths + count;
    if (int rc = stage_up<double>(c, lengths, count, [&](double &t, unsigned i) {
          t = branches[i].branch_length;
          return 0;
        }))
      return rc;
    const size_t lds = (size_t)V * (kRateRows + 1u) * sizeof(double); // 34 KB at 64 categories
    raise_lds_limit(reinterpret_cast<const void *>(&k_rate_gradient), c->device, lds);
    hipLaunchKernelGGL(k_rate_gradient, dim3(1), dim3(256), lds, c->stream, c->ins_results.p, lengths, c->rates.p, count, R, out);
    if (int rc = launched(c)) return rc;
  }
  // one copy back of everything the launches left, one wait; the caller's arrays are written last
  std::vector<double> rows(values + tail);
  if (int rc = results_down(c, rows.data(), rows.size())) return rc;
  if (host_d) memcpy(host_d, rows.data(), (size_t)count * sizeof(double));
  if (host_dd) memcpy(host_dd, rows.data() + count, (size_t)count * sizeof(double));
  if (host_d_cat)
    for (unsigned i = 0; i < count; ++i)
      for (unsigned k = 0; k < R; ++k) host_d_cat[(size_t)i * R + k] = rows[(size_t)(k + 2u) * count + i];
  if (host_d_rates) memcpy(host_d_rates, rows.data() + values + count, (size_t)R * sizeof(double));
  if (host_d_scale) *host_d_scale = rows[values + count + R];
  return 0;
}

// ---- the model gradient (kernels_qgradient.h) ------------------------------------------------------------------
constexpr unsigned kQgMaxBlocks = 64;        // workgroups per branch at most
constexpr size_t kQgLdsMax = 160 * 1024;     // k_qgradient_mfma's LDS is all dynamic
static_assert(kQgMaxBlocks == PLLGPU_QGRADIENT_MAX_BLOCKS && kQgLdsMax == PLLGPU_QGRADIENT_LDS_MAX &&
                  qg_lds_doubles(61, 2) * sizeof(double) == PLLGPU_QGRADIENT_LDS_BYTES(61, 2) &&
                  qg_lds_doubles(5, 7) * sizeof(double) == PLLGPU_QGRADIENT_LDS_BYTES(5, 7),
              "include/pll_amd_device.h states the cutting rule and the LDS a shape needs");

// The workgroups per branch and the tiles each wave (4 x 4) or workgroup walks: a function of the shape alone
// (include/pll_amd_device.h states the rule)
static TileWalk qgradient_walk(const pllgpu_ctx *c)
{
  if (c->dna_fast) return tile_walk(c, kQgMaxBlocks);
  const unsigned spad = (c->geo.states + 15u) / 16u * 16u;
  return tile_walk(c, std::min(kQgMaxBlocks, std::max(4u, 16384u / (spad * spad))));
}

// the accumulator blocks a wave of k_qgradient_mfma holds -> fn(Int<NACC>)
template <class F>
static void with_nacc(unsigned per_wave, F &&fn)
{
  if (per_wave <= 1)
    fn(Int<1>());
  else if (per_wave <= 2)
    fn(Int<2>());
  else if (per_wave <= 4)
    fn(Int<4>());
  else
    fn(Int<8>());
}

extern "C" int pllgpu_qmatrix_gradient(pllgpu_ctx_t *c, const pllgpu_branch_t *branches, unsigned count, const unsigned *params_indices,
                                       double *host_d_q, double *host_d_root)
{
  CHECK_CTX_KEEP(c);
  const pllgpu_geometry_t &g = c->geo;
  const unsigned S = g.states, SS = S * S, R = g.rate_cats;
  c->last_launches = 0;
  if (!count)
  {
    // sums over no branch
    if (host_d_q) std::fill(host_d_q, host_d_q + (size_t)g.rate_matrices * SS, 0.0);
    if (host_d_root) std::fill(host_d_root, host_d_root + (size_t)g.rate_matrices * S, 0.0);
    return 0;
  }
  static const char noun[] = "rate-matrix gradient";
  DevEdge e;
  DevDiag dg;
  if (int rc = branch_call_begin(c, branches, count, params_indices, host_d_q != nullptr, noun, e, dg)) return rc;

  // the used rate matrices in ascending order, and each category's place among them
  QGeo q;
  memset(&q, 0, sizeof q);
  std::vector<unsigned> used;
  for (unsigned m = 0; m < g.rate_matrices; ++m)
    for (unsigned k = 0; k < R; ++k)
      if (params_indices[k] == m)
      {
        q.kfirst[used.size()] = (unsigned char)k;
        used.push_back(m);
        break;
      }
  for (unsigned k = 0; k < R; ++k) q.mslot[k] = (unsigned char)(std::find(used.begin(), used.end(), params_indices[k]) - used.begin());
  q.S = S;
  q.SP = g.states_padded;
  q.SPT = c->gg.SPT;
  q.R = R;
  q.Spad = (S + 15u) / 16u * 16u;
  q.nm = (unsigned)used.size();
  const unsigned half = q.nm * SS;
  q.slot = host_d_root ? 2u * half : half;
  const unsigned nblk = q.Spad / 16u, per_wave = (R * nblk * nblk + 3u) / 4u;
  const size_t lds = qg_lds_doubles(S, R) * sizeof(double);
  if (!c->dna_fast && (lds > kQgLdsMax || per_wave > 8u))
    return fail(PLLGPU_EUNSUPPORTED, "%s: %u states x %u rate categories need %zu bytes of LDS per workgroup", noun, S, R, lds);

  const TileWalk w = qgradient_walk(c);
  const unsigned per_launch = batch_items(count, kBranchMax, q.slot, w.blocks);
  // results: W [slot], then d_q [nm][S][S] and d_root [nm][S]
  const size_t results = (size_t)q.slot + half + (size_t)q.nm * S;
  if (int rc = batch_scratch(c, e, (size_t)q.slot * per_launch * w.blocks, 0, results, (size_t)per_launch * sizeof(BranchDesc))) return rc;
  double *const W = c->ins_results.p, *const dq = W + q.slot, *const droot = dq + half;
  const double *m1 = c->pmat.p + (size_t)g.prob_matrices * c->pm_stride, *m2 = m1 + c->pm_stride;
  for (unsigned first = 0; first < count; first += per_launch)
  {
    const unsigned n = std::min(per_launch, count - first);
    if (int rc = stage_up<BranchDesc>(c, c->ins_cands.p, n, [&](BranchDesc &d, unsigned i) {
          if (int rc2 = branch_desc(c, branches[first + i], d)) return rc2;
          d.pad_ = branches[first + i].child_is_tip ? 1.0 : 0.0; // the left end is the child: H arrives transposed
          return 0;
        }))
      return rc;
    const BranchDesc *db = reinterpret_cast<const BranchDesc *>(c->ins_cands.p);
    const unsigned root_first = host_d_root && first == 0 ? 1u : 0u;
    if (c->dna_fast)
      hipLaunchKernelGGL(k_qgradient_dna, dim3(w.blocks, n), dim3(256), 0, c->stream, e, dg, q, db, m1, m2, c->ins_partials.p, w.tiles_per, root_first);
    else
    {
      const unsigned long long *tm = tipmap_ptr(c);
      with_ich(c->ich, [&](auto ICH) {
        with_nacc(per_wave, [&](auto NACC) {
          raise_lds_limit(reinterpret_cast<const void *>(&k_qgradient_mfma<ICH(), NACC()>), c->device, lds);
          hipLaunchKernelGGL((k_qgradient_mfma<ICH(), NACC()>), dim3(w.blocks, n), dim3(256), lds, c->stream, e, dg, q, db, m1, m2, c->gg, tm,
                             c->ins_partials.p, w.tiles_per, root_first);
        });
      });
    }
    if (int rc = launched(c)) return rc;
    const unsigned vblocks = (q.slot + 255u) / 256u;
    hipLaunchKernelGGL(k_qgradient_slots, dim3(vblocks, n), dim3(256), 0, c->stream, c->ins_partials.p, q.slot, half, w.blocks, root_first);
    if (int rc = launched(c)) return rc;
    hipLaunchKernelGGL(k_qgradient_branches, dim3(vblocks), dim3(256), 0, c->stream, c->ins_partials.p, W, q.slot, half, w.blocks, n,
                       first == 0 ? 1u : 0u);
    if (int rc = launched(c)) return rc;
  }
  hipLaunchKernelGGL(k_qgradient_transform, dim3(q.nm), dim3(256), (size_t)SS * sizeof(double), c->stream, W, m1, m2, c->freqs.p, q, dg,
                     host_d_root ? 1u : 0u, dq, droot);
  if (int rc = launched(c)) return rc;
  // one copy back, one wait; the caller's arrays are written last: zeros for a rate matrix that no category uses
  std::vector<double> rows(results);
  if (int rc = results_down(c, rows.data(), rows.size())) return rc;
  std::fill(host_d_q, host_d_q + (size_t)g.rate_matrices * SS, 0.0);
  if (host_d_root) std::fill(host_d_root, host_d_root + (size_t)g.rate_matrices * S, 0.0);
  for (unsigned ms = 0; ms < q.nm; ++ms)
  {
    memcpy(host_d_q + (size_t)used[ms] * SS, rows.data() + q.slot + (size_t)ms * SS, (size_t)SS * sizeof(double));
    if (host_d_root) memcpy(host_d_root + (size_t)used[ms] * S, rows.data() + q.slot + half + (size_t)ms * S, (size_t)S * sizeof(double));
  }
  return 0;
}

// ---- marginal ancestral states (kernels_ancestral.h) -------------------------------------------------------
// One launch that leaves a table per site (ancestral states here, the category likelihoods below): the 4 x 4 form or the
// tiled one of the shape, over tile_walk's table form, for a child end that is a tip or not. dna(CT, w) and
// tiled(ICH, CT, w) launch the two forms.
template <class Dna, class Tiled>
static void launch_site_table(pllgpu_ctx *c, bool ctip, Dna &&dna, Tiled &&tiled)
{
  const TileWalk w = tile_walk(c, kTableBlocks);
  with_bools(ctip, false, [&](auto CT, auto) {
    if (c->dna_fast)
      dna(CT, w);
    else
      with_ich(c->ich, [&](auto ICH) { tiled(ICH, CT, w); });
  });
}

// the call's one launch
static void launch_ancestral(pllgpu_ctx *c, const DevAncestral &a, bool ctip)
{
  launch_site_table(
      c, ctip, [&](auto CT, const TileWalk &w) { hipLaunchKernelGGL((k_ancestral_dna<CT()>), dim3(w.blocks), dim3(256), 0, c->stream, a, w.tiles_per); },
      [&](auto ICH, auto CT, const TileWalk &w) {
        const unsigned nw = tiled_waves(c);
        const size_t lds = ((size_t)nw * c->gg.S * 64u + (size_t)nw * 64u) * sizeof(double);
        raise_lds_limit(reinterpret_cast<const void *>(&k_ancestral_tiled<ICH(), CT()>), c->device, lds);
        hipLaunchKernelGGL((k_ancestral_tiled<ICH(), CT()>), dim3(w.blocks), dim3(64u * nw), lds, c->stream, a, c->gg, tipmap_ptr(c), w.tiles_per);
      });
}

extern "C" int pllgpu_node_ancestral(pllgpu_ctx_t *c, const pllgpu_edge_t *ed, double *host_out, void *device_out)
{
  CHECK_CTX(c); // (held ops and chains go out as ordinary updates first)
  const pllgpu_geometry_t &g = c->geo;
  if ((host_out == nullptr) == (device_out == nullptr)) return fail(PLLGPU_EINVAL, "ancestral states go to the host or to the device, one of the two");
  if (ed->gather) return fail(PLLGPU_EUNSUPPORTED, "ancestral states of class-compressed CLVs");
  if (int rc = check_edge(c, ed, nullptr)) return rc;
  DevAncestral a;
  if (int rc = build_edge(c, ed, a.e)) return rc;
  const size_t n = (size_t)g.sites * g.states;
  if (host_out)
    if (int rc = c->ancestral.ensure(n)) return rc;
  a.out = host_out ? c->ancestral.p : static_cast<double *>(device_out);
  for (unsigned k = 0; k < g.rate_cats; ++k) a.e.fidx[k] = (unsigned char)ed->freqs_indices[k];
  a.e.freqs = c->freqs.p;
  a.e.rate_weights = c->rate_weights.p;
  a.e.sites = g.sites;
  a.e.per_rate = g.per_rate_scalers ? 1 : 0;
  launch_ancestral(c, a, ed->child_is_tip != 0);
  ++c->last_launches;
  HIP_TRY(hipGetLastError());
  if (!host_out) return 0; // stream-ordered: the table stays where the caller asked for it
  HIP_TRY(hipMemcpyAsync(host_out, c->ancestral.p, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(stream_wait(c));
  return 0;
}

// ---- rate-category posteriors, site rates and EM weight steps (kernels_category.h) -------------------------
static_assert(PLLGPU_EM_MAX_STEPS == 1024, "include/pll_amd_device.h states the limit");

// what both calls share: the edge as stage A reads it, the model as stage B reads it, the grid of stages B and C
struct CategoryCall
{
  DevCategory a;
  DevCategoryMix m;
  unsigned blocks; // B = min(ceil(sites / 256), 1024)
  bool ctip;
};

// Every check, in the order the header states, then - the first step that touches device state - held work out and
// pending CLVs stored, the edge and the model resolved and the scratch taken. `sums`: stage B leaves partials;
// `evaluations`: how many {weight_sums, lnl} records the results buffer holds.
static int category_begin(pllgpu_ctx *c, const pllgpu_edge_t *ed, const char *noun, bool want_cat_lnl, bool want_posterior, bool want_rates, bool sums,
                          size_t evaluations, CategoryCall &k)
{
  const pllgpu_geometry_t &g = c->geo;
  if (!ed || !ed->freqs_indices) return fail(PLLGPU_EINVAL, "%s: null argument", noun);
  if (int rc = check_edge(c, ed, nullptr)) return rc;
  if (ed->gather) return fail(PLLGPU_EUNSUPPORTED, "%s of class-compressed CLVs", noun);
  if (int rc = refuse_ascertainment(c, noun)) return rc;
  if (int rc = refuse_compressed(c, noun)) return rc;
  if (want_rates && !c->rates.p) return fail(PLLGPU_EINVAL, "%s: category rates were not uploaded", noun);
  if (HOLDS_WORK(c) || !c->pending.empty())
    if (int rc = flush_deferred(c)) return rc;
  if (int rc = build_edge(c, ed, k.a.e)) return rc;
  if (int rc = fill_edge_model(c, k.a.e, ed->freqs_indices)) return rc;
  k.ctip = ed->child_is_tip != 0;
  k.blocks = std::min((g.sites + 255u) / 256u, 1024u);
  const unsigned pad = (g.sites + 63u) / 64u * 64u;
  const size_t R = g.rate_cats;
  {
    ScratchEpoch scratch_epoch_;
    if (c->cat_table.ensure(R * pad) || c->cat_count.ensure(g.sites)) return PLLGPU_ENOMEM;
    if (sums && (c->cat_partials.ensure((R + 1) * k.blocks) || c->cat_results.ensure(evaluations * (R + 1)))) return PLLGPU_ENOMEM;
    if ((want_cat_lnl && c->cat_lnl.ensure(R * g.sites)) || (want_posterior && c->cat_posterior.ensure(R * g.sites)) ||
        (want_rates && c->cat_rates.ensure(g.sites)))
      return PLLGPU_ENOMEM;
  }
  k.a.table = c->cat_table.p;
  k.a.count = c->cat_count.p;
  k.a.cat_lnl = want_cat_lnl ? c->cat_lnl.p : nullptr;
  k.a.pad = pad;

  DevCategoryMix &m = k.m;
  memset(&m, 0, sizeof m);
  m.table = c->cat_table.p;
  m.count = c->cat_count.p;
  m.weights = c->rate_weights.p;
  m.freqs = k.a.e.freqs;
  m.prop_invar = k.a.e.prop_invar;
  m.rates = c->rates.p;
  m.invariant = k.a.e.invariant;
  m.pattern_weights = k.a.e.pattern_weights;
  m.posterior = want_posterior ? c->cat_posterior.p : nullptr;
  m.site_rates = want_rates ? c->cat_rates.p : nullptr;
  m.partials = sums ? c->cat_partials.p : nullptr;
  m.sites = g.sites;
  m.pad = pad;
  m.R = g.rate_cats;
  m.SP = g.states_padded;
  memcpy(m.fidx, k.a.e.fidx, sizeof m.fidx);
  return 0;
}

// stage A
static int launch_category_table(pllgpu_ctx *c, const CategoryCall &k)
{
  launch_site_table(
      c, k.ctip, [&](auto CT, const TileWalk &w) { hipLaunchKernelGGL((k_category_dna<CT()>), dim3(w.blocks), dim3(256), 0, c->stream, k.a, w.tiles_per); },
      [&](auto ICH, auto CT, const TileWalk &w) {
        hipLaunchKernelGGL((k_category_tiled<ICH(), CT()>), dim3(w.blocks), dim3(tiled_threads(c)), 0, c->stream, k.a, c->gg, tipmap_ptr(c), w.tiles_per);
      });
  return launched(c);
}

// stages B and C of one evaluation under the weight row `weights`: its {weight_sums, lnl} to record `record` of the
// results, the row that follows to `next` (or nowhere)
static int launch_category_mix(pllgpu_ctx *c, CategoryCall &k, const double *weights, size_t record, double *next)
{
  k.m.weights = weights;
  hipLaunchKernelGGL(k_category_mix, dim3(k.blocks), dim3(256), 0, c->stream, k.m);
  if (int rc = launched(c)) return rc;
  if (!k.m.partials) return 0;
  hipLaunchKernelGGL(k_category_reduce, dim3(1), dim3(256), 0, c->stream, k.m.partials, k.blocks, k.m.R, c->cat_results.p + record * (k.m.R + 1u), next);
  return launched(c);
}

extern "C" int pllgpu_edge_category_posteriors(pllgpu_ctx_t *c, const pllgpu_edge_t *ed, double *host_cat_lnl, double *host_posterior,
                                               double *host_site_rates, double *host_weight_sums, double *host_lnl)
{
  CHECK_CTX_KEEP(c);
  const pllgpu_geometry_t &g = c->geo;
  c->last_launches = 0;
  static const char noun[] = "category posteriors";
  if (!host_cat_lnl && !host_posterior && !host_site_rates && !host_weight_sums && !host_lnl) return fail(PLLGPU_EINVAL, "%s: no output asked for", noun);
  const bool sums = host_weight_sums || host_lnl;
  CategoryCall k;
  if (int rc = category_begin(c, ed, noun, host_cat_lnl != nullptr, host_posterior != nullptr, host_site_rates != nullptr, sums, 1, k)) return rc;
  if (int rc = launch_category_table(c, k)) return rc;
  if (host_posterior || host_site_rates || sums)
    if (int rc = launch_category_mix(c, k, c->rate_weights.p, 0, nullptr)) return rc;
  // one copy back per output, one wait; the sums are handed over once everything has succeeded
  const size_t R = g.rate_cats;
  std::vector<double> record(R + 1);
  if (host_cat_lnl) HIP_TRY(hipMemcpyAsync(host_cat_lnl, c->cat_lnl.p, R * g.sites * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (host_posterior) HIP_TRY(hipMemcpyAsync(host_posterior, c->cat_posterior.p, R * g.sites * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (host_site_rates) HIP_TRY(hipMemcpyAsync(host_site_rates, c->cat_rates.p, g.sites * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (sums) HIP_TRY(hipMemcpyAsync(record.data(), c->cat_results.p, (R + 1) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(stream_wait(c));
  if (host_weight_sums) memcpy(host_weight_sums, record.data(), R * sizeof(double));
  if (host_lnl) *host_lnl = record[R];
  return 0;
}

extern "C" int pllgpu_category_weights_em(pllgpu_ctx_t *c, const pllgpu_edge_t *ed, const double *start_weights, unsigned steps, double *host_weights,
                                          double *host_lnl)
{
  CHECK_CTX_KEEP(c);
  const pllgpu_geometry_t &g = c->geo;
  c->last_launches = 0;
  static const char noun[] = "category weights EM";
  if (!start_weights || !host_weights) return fail(PLLGPU_EINVAL, "%s: null argument", noun);
  if (steps > PLLGPU_EM_MAX_STEPS) return fail(PLLGPU_EINVAL, "%s: %u steps, at most %u", noun, steps, (unsigned)PLLGPU_EM_MAX_STEPS);
  double total = 0.0;
  for (unsigned i = 0; i < g.rate_cats; ++i)
  {
    if (!(start_weights[i] >= 0.0) || !std::isfinite(start_weights[i])) return fail(PLLGPU_EINVAL, "%s: start weight %u is negative or not finite", noun, i);
    total += start_weights[i];
  }
  if (!(total > 0.0)) return fail(PLLGPU_EINVAL, "%s: the start weights sum to 0", noun);
  const size_t R = g.rate_cats, rows = (size_t)steps + 1;
  CategoryCall k;
  if (int rc = category_begin(c, ed, noun, false, false, false, true, rows, k)) return rc;
  {
    ScratchEpoch scratch_epoch_;
    if (c->cat_weights.ensure(rows * R)) return PLLGPU_ENOMEM;
  }
  HIP_TRY(copy_up(c, c->cat_weights.p, start_weights, R * sizeof(double)));
  if (int rc = launch_category_table(c, k)) return rc;
  for (size_t i = 0; i < rows; ++i)
    if (int rc = launch_category_mix(c, k, c->cat_weights.p + i * R, i, i + 1 < rows ? c->cat_weights.p + (i + 1) * R : nullptr)) return rc;
  std::vector<double> weights(rows * R), records(rows * (R + 1));
  HIP_TRY(hipMemcpyAsync(weights.data(), c->cat_weights.p, weights.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (host_lnl) HIP_TRY(hipMemcpyAsync(records.data(), c->cat_results.p, records.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(stream_wait(c));
  memcpy(host_weights, weights.data(), weights.size() * sizeof(double));
  if (host_lnl)
    for (size_t i = 0; i < rows; ++i) host_lnl[i] = records[i * (R + 1) + R];
  return 0;
}

// ---- the flat seam's tip-tip pair: the caller's lookup table in the reference's layout ---------------------
static unsigned lookup_shift(unsigned states, unsigned ncodes)
{
  if (states == 4) return 4; // 16 j + k (src/core_partials.c:1013-1071)
  unsigned sh = 0;
  while ((1u << sh) < ncodes) ++sh; // ceil(log2(maxstates)), :1152
  return sh;
}

extern "C" int pllgpu_create_lookup(pllgpu_ctx_t *c, double *lookup_host, const double *left_host, const double *right_host,
                                    const unsigned long long *tipmap_host, unsigned ncodes)
{
  CHECK_CTX(c);
  const unsigned S = c->gg.S, SP = c->gg.SP, R = c->gg.R, span = R * SP, shift = lookup_shift(S, ncodes);
  if (S == 4) ncodes = 16;
  if (!ncodes || ncodes > 256) return fail(PLLGPU_EINVAL, "lookup table over %u tip codes", ncodes);
  const size_t entries = (size_t)((ncodes - 1u) << shift) + ncodes, tab = entries * span, mat = (size_t)R * S * SP;
  if (int rc = c->scratch.ensure(tab + 2 * mat)) return rc;
  double *d_tab = c->scratch.p, *d_l = d_tab + tab, *d_r = d_l + mat;
  HIP_TRY(hipMemsetAsync(d_tab, 0, tab * sizeof(double), c->stream)); // (entries between the rows of a padded index stay 0)
  HIP_TRY(hipMemcpyAsync(d_l, left_host, mat * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d_r, right_host, mat * sizeof(double), hipMemcpyHostToDevice, c->stream));
  const unsigned long long *tm = nullptr;
  if (S != 4)
  {
    if (!tipmap_host) return fail(PLLGPU_EINVAL, "a lookup table of %u states needs the code -> state mask map", S);
    if (int rc = c->tipmap.ensure(256)) return rc;
    HIP_TRY(hipMemcpyAsync(c->tipmap.p, tipmap_host, ncodes * sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream));
    tm = c->tipmap.p;
  }
  const size_t n = (size_t)ncodes * ncodes * span;
  hipLaunchKernelGGL(k_create_lookup, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, d_tab, d_l, d_r, tm, S, SP, R, ncodes, shift);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(lookup_host, d_tab, tab * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int pllgpu_tt_from_lookup(pllgpu_ctx_t *c, double *parent_host, const unsigned char *left_codes, const unsigned char *right_codes,
                                     const double *lookup_host, unsigned sites, unsigned ncodes)
{
  CHECK_CTX(c);
  const unsigned S = c->gg.S, SP = c->gg.SP, R = c->gg.R, span = R * SP, shift = lookup_shift(S, ncodes);
  if (S == 4) ncodes = 16;
  if (!ncodes || ncodes > 256 || !sites) return fail(PLLGPU_EINVAL, "tip-tip update over %u codes, %u sites", ncodes, sites);
  for (unsigned n = 0; n < sites; ++n)
    if (left_codes[n] >= ncodes || right_codes[n] >= ncodes) return fail(PLLGPU_EINVAL, "site %u: tip code beyond the lookup table's %u codes", n, ncodes);
  const size_t entries = (size_t)((ncodes - 1u) << shift) + ncodes, tab = entries * span, out = (size_t)sites * span;
  if (int rc = c->scratch.ensure(tab + out + (2 * (size_t)sites + 7) / 8 + 1)) return rc;
  double *d_tab = c->scratch.p, *d_out = d_tab + tab;
  unsigned char *d_l = reinterpret_cast<unsigned char *>(d_out + out), *d_r = d_l + sites;
  HIP_TRY(hipMemcpyAsync(d_tab, lookup_host, tab * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d_l, left_codes, sites, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d_r, right_codes, sites, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_tt_from_lookup, dim3((unsigned)((out + 255) / 256)), dim3(256), 0, c->stream, d_out, d_tab, d_l, d_r, sites, span, shift);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(parent_host, d_out, out * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// ---- the exchange of a site-sharded run ---------------------------------------------------------
// a collective library enqueues on the context's stream from the HOST side of the boundary (group.c: ncclAllReduce):
// the calling thread's current device must be the context's while it does (its own may be another, e.g. with
// PLL_AMD_DEVICE=auto); *previous = what pllgpu_leave_device puts back, -1 = nothing to do
extern "C" int pllgpu_enter_device(pllgpu_ctx_t *c, int *previous)
{
  if (!c || !previous) return fail(PLLGPU_EINVAL, "null context");
  *previous = -1;
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess) cur = -1;
  if (cur == c->device) return 0;
  HIP_TRY(hipSetDevice(c->device));
  *previous = cur;
  return 0;
}

extern "C" void pllgpu_leave_device(int previous)
{
  if (previous >= 0) (void)hipSetDevice(previous);
}

extern "C" double *pllgpu_reduce_buffer(pllgpu_ctx_t *c)
{
  if (!c) return nullptr;
  DeviceScope device_scope_(c);
  if (device_scope_.rc || c->reduce.ensure(2)) return nullptr;
  return c->reduce.p;
}

// a rank whose evaluation failed still brings an operand to the collective (-inf poisons the sum: every rank learns
// of the failure instead of waiting inside the all-reduce)
__global__ void k_set_pair(double *__restrict__ pair, double value, double sequence)
{
  pair[0] = value;
  pair[1] = sequence;
}

extern "C" int pllgpu_reduce_poison(pllgpu_ctx_t *c, double sequence)
{
  CHECK_CTX_KEEP_PENDING(c); // (no input of a CLV)
  if (!c->reduce.p) return fail(PLLGPU_EINVAL, "no reduce buffer");
  hipLaunchKernelGGL(k_set_pair, dim3(1), dim3(1), 0, c->stream, c->reduce.p, -HUGE_VAL, sequence);
  HIP_TRY(hipGetLastError());
  return 0;
}

// value, then - once the value has been performed - the sequence word: the order the host's poll relies on
__global__ void k_publish_pair(const double *__restrict__ pair, double *__restrict__ host)
{
  const double v = pair[0], q = pair[1];
  __hip_atomic_store(host, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __hip_atomic_store(host + 1, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

extern "C" int pllgpu_reduce_fetch(pllgpu_ctx_t *c, double expected_sequence, double *value_out, int timeout_ms)
{
  CHECK_CTX_KEEP_PENDING(c); // (no input of a CLV)
  if (!c->reduce.p) return fail(PLLGPU_EINVAL, "no reduce buffer");
  // words 4 and 5 of the mapped result block (0..2 belong to the synchronous evaluations and the derivatives)
  hipLaunchKernelGGL(k_publish_pair, dim3(1), dim3(1), 0, c->stream, c->reduce.p, c->result_dev + 4);
  HIP_TRY(hipGetLastError());
  unsigned long long want;
  memcpy(&want, &expected_sequence, sizeof want);
  volatile double *res = c->result_host;
  const auto t0 = std::chrono::steady_clock::now();
  const auto arrived = [&] { return __atomic_load_n((const unsigned long long *)&res[5], __ATOMIC_ACQUIRE) == want; };
  unsigned spins = 0;
  bool slow = false;
  while (!arrived())
  {
    if (!slow)
    {
      if ((++spins & 1023u) != 0 || std::chrono::steady_clock::now() - t0 <= std::chrono::milliseconds(50)) continue;
      slow = true; // not the microseconds a collective takes: from here on look at the stream as well, and yield the core
    }
    // A collective a peer never joins does not finish, and hipStreamSynchronize on its stream would never return
    // (ADVICE r3): ask the stream instead, for a bounded time.
    const hipError_t q = hipStreamQuery(c->stream);
    if (q == hipSuccess)
    {
      if (arrived()) break;
      return fail(PLLGPU_ERUNTIME, "the reduced sequence word is %.17g, expected %.17g: the ranks are out of step", (double)res[5], expected_sequence);
    }
    if (q != hipErrorNotReady) HIP_TRY(q);
    if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(timeout_ms > 0 ? timeout_ms : 60000))
      return fail(PLLGPU_ERUNTIME, "the all-reduce did not complete within %d ms: a rank of the communicator never joined it (the partition's stream stays blocked behind the collective)",
                  timeout_ms > 0 ? timeout_ms : 60000);
    std::this_thread::sleep_for(std::chrono::microseconds(200));
  }
  *value_out = c->result_host[4];
  return 0;
}

// ---- stream / timing ---------------------------------------------------------------------------
extern "C" int pllgpu_set_stream(pllgpu_ctx_t *c, void *s)
{
  CHECK_CTX(c);
  HIP_TRY(stream_wait(c));
  if (c->own_stream) (void)hipStreamDestroy(c->stream);
  c->stream = (hipStream_t)s;
  c->own_stream = false;
  return 0;
}

extern "C" void *pllgpu_get_stream(const pllgpu_ctx_t *cc)
{
  // a caller who asks for the stream is about to order its own work against ours: nothing may be held back
  pllgpu_ctx *c = const_cast<pllgpu_ctx *>(cc);
  if (c && (HOLDS_WORK(c) || !c->pending.empty()))
  {
    DeviceScope device_scope_(c);
    if (device_scope_.rc == 0) (void)flush_deferred(c);
  }
  return c ? (void *)c->stream : nullptr;
}

extern "C" int pllgpu_synchronize(pllgpu_ctx_t *c)
{
  CHECK_CTX_KEEP_PENDING(c); // pending CLVs are a representation, not work in flight
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int pllgpu_timer_start(pllgpu_ctx_t *c)
{
  CHECK_CTX_KEEP_PENDING(c); // (no input of a CLV)
  HIP_TRY(hipEventRecord(c->ev0, c->stream));
  return 0;
}

extern "C" double pllgpu_timer_stop(pllgpu_ctx_t *c)
{
  if (!c) return -1.0;
  DeviceScope device_scope_(c);
  if (device_scope_.rc) return -1.0;
  if (HOLDS_WORK(c) && flush_deferred(c, true)) return -1.0; // the timer reads no CLV
  float ms = 0;
  if (hipEventRecord(c->ev1, c->stream) != hipSuccess || hipEventSynchronize(c->ev1) != hipSuccess ||
      hipEventElapsedTime(&ms, c->ev0, c->ev1) != hipSuccess)
  {
    fail(PLLGPU_ERUNTIME, "event timing failed");
    return -1.0;
  }
  return (double)ms;
}

// ---- maximum-likelihood distances between tips (kernels_distance.h) ------------------------------------------------
// the private count tables of a workgroup: as many as fit kDistCountBytes (a power of two, at most one per thread), one at
// least; an odd number of words apart
constexpr size_t kDistCountBytes = 36 * 1024;

static const char kDistNoun[] = "pairwise distances";

// the checks of the arguments themselves (count > 0), in the order include/pll_amd_device.h states
static int distances_check_arguments(pllgpu_ctx *c, const unsigned *tips, unsigned count, const unsigned *params_indices, const pllgpu_newton_t *opt)
{
  const char *const noun = kDistNoun;
  const pllgpu_geometry_t &g = c->geo;
  if (!tips || !params_indices || !opt) return fail(PLLGPU_EINVAL, "%s: null argument", noun);
  for (unsigned i = 0; i < count; ++i)
    if (tips[i] >= g.tips) return fail(PLLGPU_EINVAL, "%s: tips[%u] = %u is no tip", noun, i, tips[i]);
  if (!(opt->t_min >= 0) || !(opt->t_min <= opt->t_max) || !std::isfinite(opt->t_max) || !std::isfinite(opt->t_start) || !(opt->tolerance > 0) ||
      opt->max_iters < 1 || opt->max_iters > PLLGPU_NEWTON_MAX_ITERS || opt->matrix_index != -1)
    return fail(PLLGPU_EINVAL, "%s: options out of range", noun);
  return check_rate_indices(c, "params_indices", params_indices);
}

// The remaining checks of a list of tips: what the context holds for them
static int distances_check_state(const pllgpu_ctx *c, const unsigned *tips, unsigned count)
{
  const char *const noun = kDistNoun;
  const pllgpu_geometry_t &g = c->geo;
  for (unsigned i = 0; i < count; ++i)
    if (!c->tipchars[tips[i]].p) return fail(PLLGPU_EINVAL, "%s: tip %u has no codes on the device", noun, tips[i]);
  if (int rc = refuse_ascertainment(c, noun)) return rc;
  if (int rc = refuse_compressed(c, noun)) return rc;
  const unsigned S = g.states, R = g.rate_cats;
  const unsigned ncodes = S == 4 ? 16u : c->tip_ncodes;
  if (ncodes > PLLGPU_DISTANCE_MAX_CODES || PLLGPU_DISTANCE_LDS_BYTES((size_t)S, (size_t)R, (size_t)ncodes) > PLLGPU_DISTANCE_LDS_MAX)
    return fail(PLLGPU_EUNSUPPORTED, "%s: a code table of %u codes at %u states x %u rate categories (at most %u codes and %lu bytes of LDS)", noun, ncodes,
                S, R, (unsigned)PLLGPU_DISTANCE_MAX_CODES, PLLGPU_DISTANCE_LDS_MAX);
  if (!ncodes || (S != 4 && !c->tipmap_set)) return fail(PLLGPU_EINVAL, "%s: the code -> state mask map was not uploaded", noun);
  if (!c->eigenvals.p || !c->rates.p) return fail(PLLGPU_EINVAL, "eigenvalues / category rates were not uploaded");
  return 0;
}

// what the pair launches of a call share
struct DistanceCall
{
  DevDistance d;
  DevDiag dg;
  size_t lds;
};

// Once per call, behind the checks: held work goes out, the scratch for `blocks` result blocks of 6 count^2 values, the code
// rows of the list and ONE launch of k_distance_code_vectors.
static int distances_begin(pllgpu_ctx *c, const unsigned *tips, unsigned count, const unsigned *params_indices, const pllgpu_newton_t *opt, size_t blocks,
                           DistanceCall &k)
{
  const pllgpu_geometry_t &g = c->geo;
  const unsigned S = g.states, R = g.rate_cats;
  const unsigned ncodes = S == 4 ? 16u : c->tip_ncodes;
  const size_t diag_bytes = (size_t)R * S * 4 * sizeof(double);
  DevEdge e;
  if (int rc = batch_edge(c, e, params_indices)) return rc;

  const size_t cc = (size_t)count * count, uw = (size_t)2 * ncodes * R * S;
  if (int rc = batch_scratch(c, e, uw, 0, blocks * 6 * cc, (size_t)count * sizeof(const unsigned char *))) return rc;
  const int up = stage_up<const unsigned char *>(c, c->ins_cands.p, count, [&](const unsigned char *&row, unsigned i) {
    row = c->tipchars[tips[i]].p;
    return 0;
  });
  if (up) return up;

  const double *m1 = c->pmat.p + (size_t)g.prob_matrices * c->pm_stride, *m2 = m1 + c->pm_stride;
  const unsigned long long *tm = S == 4 ? nullptr : c->tipmap.p;
  hipLaunchKernelGGL(k_distance_code_vectors, dim3((unsigned)((uw + 255) / 256)), dim3(256), 0, c->stream, m1, m2, tm, ncodes, S, c->gg.SPT, R,
                     c->ins_partials.p);
  if (int rc = launched(c)) return rc;

  DevDiag &dg = k.dg;
  memset(&dg, 0, sizeof dg);
  for (unsigned r = 0; r < R; ++r) dg.fidx[r] = (unsigned char)params_indices[r];
  dg.eigenvals = c->eigenvals.p;
  dg.rates = c->rates.p;
  dg.prop_invar = c->prop_invar.p;
  dg.S = S;
  dg.SP = g.states_padded;
  dg.R = R;
  DevDistance &d = k.d;
  memset(&d, 0, sizeof d);
  d.rows = reinterpret_cast<const unsigned char *const *>(c->ins_cands.p);
  d.pattern_weights = e.pattern_weights;
  d.uw = c->ins_partials.p;
  d.tipmap = tm;
  d.freqs = e.freqs;
  d.rate_weights = e.rate_weights;
  d.results = c->ins_results.p;
  d.t_first = std::min(std::max(opt->t_start, opt->t_min), opt->t_max);
  d.t_min = opt->t_min;
  d.t_max = opt->t_max;
  d.tolerance = opt->tolerance;
  d.max_iters = opt->max_iters;
  d.sites = g.sites;
  d.count = count;
  d.ncodes = ncodes;
  d.copy_stride = (ncodes * ncodes) | 1u;
  const size_t table = (size_t)d.copy_stride * sizeof(unsigned);
  const size_t room = std::min<size_t>(std::max(kDistCountBytes, table), PLLGPU_DISTANCE_LDS_MAX - diag_bytes);
  d.copies = 1u;
  while (d.copies < 256u && (size_t)2 * d.copies * table <= room) d.copies *= 2u;
  memcpy(d.fidx, e.fidx, sizeof d.fidx);
  k.lds = diag_bytes + (size_t)d.copies * table;
  raise_lds_limit(reinterpret_cast<const void *>(&k_pairwise_distances), c->device, k.lds);
  raise_lds_limit(reinterpret_cast<const void *>(&k_pairwise_distances_rows), c->device, k.lds);
  return 0;
}

// The pair launches of `nr` result blocks, the first nr of ins_results, with nothing waited for. wrows == nullptr: the one
// block under the context's pattern weights (k_pairwise_distances). Else block z under row z of wrows, wstride words apart
// (k_pairwise_distances_rows). The cutting rule (include/pll_amd_device.h states it): a launch holds at most distance_pairs
// workgroups, cells x replicates - whole matrices of as many replicates as fit or, where one matrix does not fit, whole
// rows of one replicate's.
static int distances_launch(pllgpu_ctx *c, DistanceCall &k, const unsigned *wrows, unsigned wstride, unsigned nr)
{
  DevDistance &d = k.d;
  const unsigned count = d.count;
  HIP_TRY(hipMemsetAsync(c->ins_results.p, 0, (size_t)nr * 6 * count * count * sizeof(double), c->stream)); // the diagonals
  const unsigned rows_per = std::max(1u, std::min(65535u, c->distance_pairs / count));
  if (!wrows)
  {
    for (unsigned row0 = 0; row0 + 1 < count; row0 += rows_per)
    {
      d.row0 = row0;
      hipLaunchKernelGGL(k_pairwise_distances, dim3(count, std::min(rows_per, count - 1 - row0)), dim3(256), k.lds, c->stream, d, k.dg);
      if (int rc = launched(c)) return rc;
    }
    return 0;
  }
  d.pattern_weights = wrows;
  d.wstride = wstride;
  const bool whole = rows_per >= count - 1;
  const unsigned reps_per = whole ? std::max(1u, std::min(65535u, c->distance_pairs / (count * (count - 1)))) : 1u;
  for (unsigned rep0 = 0; rep0 < nr; rep0 += reps_per)
    for (unsigned row0 = 0; row0 + 1 < count; row0 += rows_per)
    {
      d.rep0 = rep0;
      d.row0 = row0;
      hipLaunchKernelGGL(k_pairwise_distances_rows, dim3(count, std::min(rows_per, count - 1 - row0), std::min(reps_per, nr - rep0)), dim3(256), k.lds,
                         c->stream, d, k.dg);
      if (int rc = launched(c)) return rc;
    }
  return 0;
}

// The remaining checks and every launch of a list of count >= 2 tips: the six [count][count] blocks are left in
// ins_results, distance first, with nothing waited for. pllgpu_pairwise_distances copies them back; pllgpu_distance_tree
// joins the first block where it lies.
static int distances_enqueue(pllgpu_ctx *c, const unsigned *tips, unsigned count, const unsigned *params_indices, const pllgpu_newton_t *opt)
{
  if (int rc = distances_check_state(c, tips, count)) return rc;
  DistanceCall k;
  if (int rc = distances_begin(c, tips, count, params_indices, opt, 1, k)) return rc;
  return distances_launch(c, k, nullptr, 0, 1);
}

extern "C" int pllgpu_pairwise_distances(pllgpu_ctx_t *c, const unsigned *tips, unsigned count, const unsigned *params_indices,
                                         const pllgpu_newton_t *opt, const pllgpu_distances_t *out)
{
  CHECK_CTX_KEEP(c);
  c->last_launches = 0;
  if (!out || !out->distance) return fail(PLLGPU_EINVAL, "%s: null argument", kDistNoun);
  if (!count) return 0;
  if (int rc = distances_check_arguments(c, tips, count, params_indices, opt)) return rc;
  if (count == 1)
  {
    // no pair: the one diagonal entry
    out->distance[0] = 0.0;
    if (out->p_distance) out->p_distance[0] = 0.0;
    if (out->d_f) out->d_f[0] = 0.0;
    if (out->dd_f) out->dd_f[0] = 0.0;
    if (out->status) out->status[0] = 0;
    if (out->iterations) out->iterations[0] = 0u;
    return 0;
  }
  if (int rc = distances_enqueue(c, tips, count, params_indices, opt)) return rc;
  const size_t cc = (size_t)count * count;
  std::vector<double> host(6 * cc);
  if (int rc = results_down(c, host.data(), host.size())) return rc;
  memcpy(out->distance, host.data(), cc * sizeof(double));
  if (out->p_distance) memcpy(out->p_distance, host.data() + cc, cc * sizeof(double));
  if (out->d_f) memcpy(out->d_f, host.data() + 2 * cc, cc * sizeof(double));
  if (out->dd_f) memcpy(out->dd_f, host.data() + 3 * cc, cc * sizeof(double));
  if (out->status)
    for (size_t i = 0; i < cc; ++i) out->status[i] = (int)host[4 * cc + i];
  if (out->iterations)
    for (size_t i = 0; i < cc; ++i) out->iterations[i] = (unsigned)host[5 * cc + i];
  return 0;
}

// ---- neighbour-joining / BIONJ trees (kernels_nj.h) -------------------------------------------------------------------
constexpr unsigned kNjRows = PLLGPU_NJ_ROWS; // rows of the triangle per search workgroup; PLL_AMD_NJ_ROWS lowers it (tests)
static thread_local unsigned t_nj_launches = 0;
static thread_local double t_nj_device_ms = -1.0; // first to last launch of this thread's last join, by device events

static unsigned nj_rows()
{
  unsigned rows = kNjRows;
  if (const char *v = getenv("PLL_AMD_NJ_ROWS")) // tests: a small matrix over several search workgroups and the ticket
    rows = (unsigned)std::min<long>(std::max<long>(1, atol(v)), (long)kNjRows);
  return rows;
}

// bytes of a replicate's working set behind a 256-byte aligned block - the stride from one replicate's to the next one's -
// and the block cut up. The tickets and the status word lie side by side: one memset serves both.
static size_t nj_align(size_t b) { return (b + 255u) & ~(size_t)255u; }
static size_t nj_zeroed_bytes(unsigned count) { return nj_align((size_t)count * sizeof(unsigned)) + sizeof(unsigned); }
static size_t nj_scratch_bytes(unsigned count, unsigned flags)
{
  const size_t n = count, cc = n * n * sizeof(double);
  return nj_align(cc) * ((flags & PLLGPU_NJ_BIONJ) ? 2u : 1u) + nj_align(n * sizeof(double)) + nj_align(4 * n * sizeof(double)) +
         2 * nj_align(n * sizeof(unsigned)) + nj_align(n * sizeof(NjKey)) + nj_align(sizeof(NjRecord)) + nj_align(2 * n * sizeof(int)) +
         nj_align(2 * n * sizeof(double)) + nj_align(sizeof(unsigned));
}

extern "C" size_t pllgpu_nj_scratch_bytes(unsigned count, unsigned flags) { return nj_scratch_bytes(count, flags); }

// replicate 0's working set at `block`; src_stride: doubles between the input matrices
static DevNj nj_carve(unsigned char *block, unsigned count, unsigned flags, unsigned rows, size_t src_stride)
{
  const size_t n = count, cc = n * n * sizeof(double);
  DevNj d;
  memset(&d, 0, sizeof d);
  auto take = [&](size_t bytes) {
    unsigned char *p = block;
    block += nj_align(bytes);
    return p;
  };
  d.D = (double *)take(cc);
  d.V = (flags & PLLGPU_NJ_BIONJ) ? (double *)take(cc) : nullptr;
  d.R = (double *)take(n * sizeof(double));
  d.snap = (double *)take(4 * n * sizeof(double));
  d.label = (unsigned *)take(n * sizeof(unsigned));
  d.partials = (NjKey *)take(n * sizeof(NjKey));
  d.record = (NjRecord *)take(sizeof(NjRecord));
  d.parent = (int *)take(2 * n * sizeof(int));
  d.length = (double *)take(2 * n * sizeof(double));
  d.tickets = (unsigned *)take(n * sizeof(unsigned));
  d.status = (unsigned *)take(sizeof(unsigned));
  d.stride = nj_scratch_bytes(count, flags);
  d.src_stride = src_stride;
  d.count = count;
  d.rows = rows;
  d.bionj = (flags & PLLGPU_NJ_BIONJ) ? 1u : 0u;
  return d;
}

// what a batch of joins leaves on the host once its stream has been waited for
struct NjBatch
{
  std::vector<int> parent;
  std::vector<double> length;
  std::vector<unsigned> status;
  // (the two events time the launches for tools/nj_probe.py; when they cannot be had the call runs without them)
  hipEvent_t first = nullptr, last = nullptr;
  bool timed = false;
  ~NjBatch()
  {
    if (first) (void)hipEventDestroy(first);
    if (last) (void)hipEventDestroy(last);
  }
};

// rows of `width` bytes, `nr` of them a replicate's stride apart on the device, to a dense host array: one copy
static hipError_t nj_rows_down(hipStream_t stream, void *host, const void *dev, size_t width, size_t stride, unsigned nr)
{
  if (nr == 1) return hipMemcpyAsync(host, dev, width, hipMemcpyDeviceToHost, stream);
  return hipMemcpy2DAsync(host, width, dev, stride, width, nr, hipMemcpyDeviceToHost, stream);
}

// The one routine behind every call, first half: the joins of the nr <= 65535 device matrices src, src + src_stride, ...
// ([count][count] each, the upper triangle read) in lockstep on `stream`, in `block` (nr x nj_scratch_bytes of it), the
// replicate the grids' second dimension; then parents, lengths and status words on their way to `out` in one copy each.
// Nothing is waited for. Launches (the rule of include/pll_amd_device.h: they do not depend on nr) are added to *launches.
static int nj_enqueue(hipStream_t stream, const double *src, size_t src_stride, unsigned nr, unsigned count, unsigned flags, unsigned char *block,
                      NjBatch &out, unsigned *launches)
{
  const DevNj d = nj_carve(block, count, flags, nj_rows(), src_stride);
  const size_t nodes = 2 * (size_t)count - 2;
  t_nj_device_ms = -1.0;
  if (hipEventCreate(&out.first) != hipSuccess || hipEventCreate(&out.last) != hipSuccess) (void)hipGetLastError();
  // every replicate's tickets and status word
  if (nr == 1) HIP_TRY(hipMemsetAsync(d.tickets, 0, nj_zeroed_bytes(count), stream));
  else HIP_TRY(hipMemset2DAsync(d.tickets, d.stride, 0, nj_zeroed_bytes(count), nr, stream));
  const bool timed = out.first && out.last && hipEventRecord(out.first, stream) == hipSuccess;
  if (count == 3)
  {
    hipLaunchKernelGGL(k_nj_final, dim3(1, nr), dim3(64), 0, stream, d, src);
    ++*launches;
  }
  else
  {
    hipLaunchKernelGGL(k_nj_init, dim3(count, nr), dim3(256), 0, stream, d, src);
    ++*launches;
    for (unsigned r = count, step = 0; r > 3; --r, ++step)
    {
      const unsigned search_wgs = (r - 1 + d.rows - 1) / d.rows; // rows 0 .. r-2 of the triangle hold pairs
      hipLaunchKernelGGL(k_nj_search, dim3(search_wgs, nr), dim3(256), 0, stream, d, r, step);
      hipLaunchKernelGGL(k_nj_join, dim3((r + 255) / 256, nr), dim3(256), 0, stream, d, r, step);
      *launches += 2;
    }
    hipLaunchKernelGGL(k_nj_final, dim3(1, nr), dim3(64), 0, stream, d, (const double *)nullptr);
    ++*launches;
  }
  HIP_TRY(hipGetLastError());
  out.timed = timed && hipEventRecord(out.last, stream) == hipSuccess;
  out.parent.resize(nr * nodes);
  out.length.resize(nr * nodes);
  out.status.assign(nr, 0u);
  HIP_TRY(nj_rows_down(stream, out.parent.data(), d.parent, nodes * sizeof(int), d.stride, nr));
  HIP_TRY(nj_rows_down(stream, out.length.data(), d.length, nodes * sizeof(double), d.stride, nr));
  HIP_TRY(nj_rows_down(stream, out.status.data(), d.status, sizeof(unsigned), d.stride, nr));
  return 0;
}

// ... second half, once the stream has been waited for: the trees into parent / length ([nr][2 count - 2] each), unless a
// replicate's search found no pair; `first` is replicate 0's number in the call
static int nj_finish(NjBatch &b, unsigned first, int *parent, double *length)
{
  float ms = 0;
  if (b.timed && hipEventElapsedTime(&ms, b.first, b.last) == hipSuccess) t_nj_device_ms = (double)ms;
  for (size_t r = 0; r < b.status.size(); ++r)
    if (b.status[r])
      return fail(PLLGPU_ERUNTIME, "neighbour joining: a step of replicate %u found no pair to join (the criterion is not a number)", first + (unsigned)r);
  memcpy(parent, b.parent.data(), b.parent.size() * sizeof(int));
  memcpy(length, b.length.data(), b.length.size() * sizeof(double));
  return 0;
}

static int nj_run(hipStream_t stream, const double *src, size_t src_stride, unsigned nr, unsigned first, unsigned count, unsigned flags,
                  unsigned char *block, int *parent, double *length, unsigned *launches)
{
  NjBatch b;
  if (int rc = nj_enqueue(stream, src, src_stride, nr, count, flags, block, b, launches)) return rc;
  HIP_TRY(hipStreamSynchronize(stream));
  return nj_finish(b, first, parent, length);
}

extern "C" unsigned pllgpu_nj_last_launch_count(void) { return t_nj_launches; }
extern "C" double pllgpu_nj_last_device_ms(void) { return t_nj_device_ms; }

extern "C" int pllgpu_nj_trees(int device, const double *host_dist, unsigned count, unsigned replicates, unsigned flags, int *parent, double *length)
{
  t_nj_launches = 0;
  if (!host_dist || !parent || !length || count < 3 || (flags & ~PLLGPU_NJ_BIONJ))
    return fail(PLLGPU_EINVAL, "neighbour joining: invalid argument (%u nodes, flags %#x)", count, flags);
  if (!replicates) return 0;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
  {
    (void)hipGetLastError();
    return fail(PLLGPU_ENODEVICE, "no HIP device visible");
  }
  int prev = -1;
  if (hipGetDevice(&prev) != hipSuccess) prev = -1;
  if (device < 0)
  {
    // PLL_AMD_DEVICE=<n>, else (unset or "auto") the calling thread's current device - like pllgpu_compress_patterns
    const char *env = getenv("PLL_AMD_DEVICE");
    device = (env && strcmp(env, "auto") != 0) ? atoi(env) : (prev >= 0 ? prev : 0);
  }
  if (device < 0 || device >= ndev) return fail(PLLGPU_EINVAL, "neighbour joining: device %d of %d", device, ndev);
  // the chunks: matrices and working sets of one stay under the budget
  size_t budget = PLLGPU_NJ_BATCH_MAX_BYTES;
  if (const char *v = getenv("PLL_AMD_NJ_BATCH_BYTES")) // tests: a few small matrices over several chunks
    if (atoll(v) >= 1) budget = std::min<size_t>((size_t)atoll(v), PLLGPU_NJ_BATCH_MAX_BYTES);
  const size_t cc = (size_t)count * count, nodes = 2 * (size_t)count - 2, scratch = nj_scratch_bytes(count, flags);
  const unsigned per_chunk = (unsigned)std::min<size_t>(std::min(replicates, 65535u), std::max<size_t>(1, budget / (cc * sizeof(double) + scratch)));
  hipStream_t stream = nullptr;
  unsigned char *block = nullptr;
  double *src = nullptr;
  unsigned launches = 0;
  // (several chunks: the outputs are written once every one has succeeded)
  std::vector<int> hp(per_chunk < replicates ? replicates * nodes : 0);
  std::vector<double> hl(hp.size());
  auto run = [&]() -> int {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    HIP_TRY(hipMalloc(&src, per_chunk * cc * sizeof(double)));
    HIP_TRY(hipMalloc(&block, per_chunk * scratch));
    for (unsigned r0 = 0; r0 < replicates; r0 += per_chunk)
    {
      const unsigned nr = std::min(per_chunk, replicates - r0);
      HIP_TRY(hipMemcpyAsync(src, host_dist + r0 * cc, nr * cc * sizeof(double), hipMemcpyHostToDevice, stream));
      int *p = hp.empty() ? parent : hp.data() + r0 * nodes;
      double *l = hl.empty() ? length : hl.data() + r0 * nodes;
      if (int rc = nj_run(stream, src, cc, nr, r0, count, flags, block, p, l, &launches)) return rc;
    }
    return 0;
  };
  const int rc = run();
  if (rc && stream) (void)hipStreamSynchronize(stream); // nothing of the call is in flight when its blocks go
  (void)hipFree(src);
  (void)hipFree(block);
  if (stream) (void)hipStreamDestroy(stream);
  if (rc) (void)hipGetLastError();
  if (prev >= 0 && prev != device) (void)hipSetDevice(prev); // leave the thread's device as found
  t_nj_launches = rc ? 0 : launches;
  if (!rc && !hp.empty())
  {
    memcpy(parent, hp.data(), hp.size() * sizeof(int));
    memcpy(length, hl.data(), hl.size() * sizeof(double));
  }
  return rc;
}

extern "C" int pllgpu_nj_tree(int device, const double *host_dist, unsigned count, unsigned flags, int *parent, double *length)
{
  return pllgpu_nj_trees(device, host_dist, count, 1, flags, parent, length);
}

extern "C" int pllgpu_distance_tree(pllgpu_ctx_t *c, const unsigned *tips, unsigned count, const unsigned *params_indices,
                                    const pllgpu_newton_t *opt, unsigned flags, int *parent, double *length, double *host_dist)
{
  CHECK_CTX_KEEP(c);
  c->last_launches = 0;
  if (!parent || !length) return fail(PLLGPU_EINVAL, "distance tree: null argument");
  if (count)
    if (int rc = distances_check_arguments(c, tips, count, params_indices, opt)) return rc;
  if (count < 3 || (flags & ~PLLGPU_NJ_BIONJ)) return fail(PLLGPU_EINVAL, "distance tree: invalid argument (%u tips, flags %#x)", count, flags);
  if (int rc = distances_enqueue(c, tips, count, params_indices, opt)) return rc;
  // the working set comes from the context's block pool and goes back to it; no kept plan points at it
  ScratchEpoch scratch_epoch_;
  DevBuf<unsigned char> block;
  if (block.ensure(nj_scratch_bytes(count, flags))) return PLLGPU_ENOMEM;
  std::vector<double> dist;
  int rc = 0;
  if (host_dist)
  {
    dist.resize((size_t)count * count);
    const hipError_t e = hipMemcpyAsync(dist.data(), c->ins_results.p, dist.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e != hipSuccess) rc = fail(PLLGPU_ERUNTIME, "distance tree: copy back failed: %s", hipGetErrorString(e));
  }
  unsigned launches = 0;
  if (!rc) rc = nj_run(c->stream, c->ins_results.p, 0, 1, 0, count, flags, block.p, parent, length, &launches);
  if (rc) (void)hipStreamSynchronize(c->stream);
  else ring_drained(c); // (nj_run has waited for the stream)
  block.release();
  if (rc) return rc;
  c->last_launches += launches;
  if (host_dist) memcpy(host_dist, dist.data(), dist.size() * sizeof(double));
  return 0;
}

// ---- bootstrap trees from distances ---------------------------------------------------------
// Per chunk of replicates, on the context's stream with no host wait inside: k_rell_draw into rows of rs_w, the pair
// launches under those rows into a chunk's result blocks, the joins of the distance planes where they lie, the copies back
// that were asked for, one wait. The cut and the launch rule: include/pll_amd_device.h.
extern "C" int pllgpu_bootstrap_distance_trees(pllgpu_ctx_t *c, const unsigned *tips, unsigned count, const unsigned *params_indices,
                                               const pllgpu_newton_t *opt, unsigned flags, unsigned long long seed, unsigned first,
                                               unsigned replicates, const pllgpu_bootstrap_trees_t *out)
{
  CHECK_CTX_KEEP(c);
  static const char noun[] = "bootstrap distance trees";
  c->last_launches = 0;
  if (!out || !out->parent || !out->length) return fail(PLLGPU_EINVAL, "%s: null argument", noun);
  if (!replicates) return 0;
  if (count)
    if (int rc = distances_check_arguments(c, tips, count, params_indices, opt)) return rc;
  if (count < 3 || (flags & ~PLLGPU_NJ_BIONJ)) return fail(PLLGPU_EINVAL, "%s: invalid argument (%u tips, flags %#x)", noun, count, flags);
  if (int rc = distances_check_state(c, tips, count)) return rc;
  if (int rc = rell_cdf_current(c)) return rc;
  if (int rc = rell_check_total(c, noun)) return rc;

  const unsigned sites = c->geo.sites, wstride = (sites + 3u) / 4u * 4u;
  const size_t cc = (size_t)count * count, nodes = 2 * (size_t)count - 2, scratch = nj_scratch_bytes(count, flags);
  const size_t per_replicate = (size_t)wstride * sizeof(unsigned) + 6 * cc * sizeof(double) + scratch;
  const unsigned per_chunk = (unsigned)std::min<size_t>(std::min(replicates, 65535u), std::max<size_t>(1, c->bootstrap_bytes / per_replicate));
  DistanceCall k;
  if (int rc = distances_begin(c, tips, count, params_indices, opt, per_chunk, k)) return rc;
  ScratchEpoch scratch_epoch_;
  DevBuf<unsigned char> block;
  // whatever ends the call, the chunk's blocks go back to the pool once nothing of it is in flight
  struct GiveBack
  {
    pllgpu_ctx *c;
    DevBuf<unsigned char> &block;
    bool waited = false;
    ~GiveBack()
    {
      if (!waited) (void)hipStreamSynchronize(c->stream);
      block.release();
      c->rs_w.release();
      c->ins_results.release();
    }
  } give_back{c, block};
  if (block.ensure(per_chunk * scratch) || c->rs_w.ensure((size_t)per_chunk * wstride)) return PLLGPU_ENOMEM;
  if (int rc = resample_events(c)) return rc;
  std::vector<double> dist(out->distances ? per_chunk * cc : 0), status(out->status ? per_chunk * cc : 0);
  const size_t plane = cc * sizeof(double);

  for (unsigned r0 = 0; r0 < replicates; r0 += per_chunk)
  {
    const unsigned nr = std::min(per_chunk, replicates - r0);
    const bool timed = r0 == 0;
    give_back.waited = false;
    if (timed) HIP_TRY(hipEventRecord(c->rs_ev[0], c->stream));
    if (int rc = launch_rell_draw(c, seed, first + r0, nr, wstride)) return rc;
    if (timed) HIP_TRY(hipEventRecord(c->rs_ev[1], c->stream));
    if (int rc = distances_launch(c, k, c->rs_w.p, wstride, nr)) return rc;
    if (timed) HIP_TRY(hipEventRecord(c->rs_ev[2], c->stream));
    NjBatch trees;
    unsigned launches = 0;
    if (int rc = nj_enqueue(c->stream, c->ins_results.p, 6 * cc, nr, count, flags, block.p, trees, &launches)) return rc;
    if (timed) HIP_TRY(hipEventRecord(c->rs_ev[3], c->stream));
    // plane 0 (the distances) and plane 4 (the status words) of every replicate's block: one copy each
    if (out->distances) HIP_TRY(hipMemcpy2DAsync(dist.data(), plane, c->ins_results.p, 6 * plane, plane, nr, hipMemcpyDeviceToHost, c->stream));
    if (out->status)
      HIP_TRY(hipMemcpy2DAsync(status.data(), plane, c->ins_results.p + 4 * cc, 6 * plane, plane, nr, hipMemcpyDeviceToHost, c->stream));
    if (out->weights)
    {
      if (int rc = rell_rows_down(c, out->weights + (size_t)r0 * sites, nr, wstride)) return rc; // (its wait is the chunk's)
    }
    else
      HIP_TRY(stream_wait(c));
    give_back.waited = true;
    if (int rc = nj_finish(trees, r0, out->parent + r0 * nodes, out->length + r0 * nodes)) return rc;
    c->last_launches += launches;
    if (out->distances) memcpy(out->distances + r0 * cc, dist.data(), nr * plane);
    if (out->status)
      for (size_t i = 0; i < nr * cc; ++i) out->status[r0 * cc + i] = (int)status[i];
    if (timed)
      for (int t = 0; t < 3; ++t)
      {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, c->rs_ev[t], c->rs_ev[t + 1]));
        c->bs_ms[t] = (double)ms;
      }
  }
  return 0;
}

extern "C" int pllgpu_bootstrap_last_times(const pllgpu_ctx_t *c, double *ms)
{
  if (!c || !ms) return fail(PLLGPU_EINVAL, "null argument");
  for (int t = 0; t < 3; ++t) ms[t] = c->bs_ms[t];
  return 0;
}

extern "C" unsigned pllgpu_last_launch_count(const pllgpu_ctx_t *c) { return c ? c->last_launches : 0; }
extern "C" unsigned long long pllgpu_plan_replays(const pllgpu_ctx_t *c) { return c ? c->plan_replays : 0ull; }
extern "C" unsigned long long pllgpu_class_map_work(const pllgpu_ctx_t *c, int launches)
{
  if (!c) return 0ull;
  return launches == 2 ? c->rep_calls_total : launches ? c->rep_launches_total : c->rep_ops_total;
}

// ---- branch-length derivatives ------------------------------------------------------------------
extern "C" int pllgpu_eigenvals_upload(pllgpu_ctx_t *c, unsigned index, const double *host)
{
  CHECK_CTX_KEEP_PENDING(c); // (no input of a CLV)
  if (index >= c->geo.rate_matrices) return fail(PLLGPU_EINVAL, "eigenvalue set %u out of range", index);
  if (int rc = c->eigenvals.ensure((size_t)c->geo.rate_matrices * c->geo.states_padded)) return rc;
  HIP_TRY(hipMemcpyAsync(c->eigenvals.p + (size_t)index * c->geo.states_padded, host,
                         c->geo.states_padded * sizeof(double), hipMemcpyHostToDevice, c->stream));
  return 0;
}

extern "C" int pllgpu_rates_upload(pllgpu_ctx_t *c, const double *host)
{
  CHECK_CTX_KEEP_PENDING(c); // (no input of a CLV)
  if (int rc = c->rates.ensure(c->geo.rate_cats)) return rc;
  HIP_TRY(hipMemcpyAsync(c->rates.p, host, c->geo.rate_cats * sizeof(double), hipMemcpyHostToDevice, c->stream));
  return 0;
}

static int sumtable_slot(pllgpu_ctx *c, unsigned slot)
{
  if (slot >= PLLGPU_SUMTABLE_SLOTS) return fail(PLLGPU_EINVAL, "sumtable slot %u out of range", slot);
  return c->sumtable[slot].ensure(clv_elems(c, c->geo.sites_alloc));
}

extern "C" int pllgpu_update_sumtable(pllgpu_ctx_t *c, const pllgpu_sumtable_t *st, unsigned slot)
{
  // reads the two ends of its edge: pending CLVs are stored first only if an end is one (a Newton pass on the root edge
  // after a step leaves them as they are)
  CHECK_CTX_KEEP_PENDING(c);
  const pllgpu_geometry_t &g = c->geo;
  if (st->left_clv >= g.nodes || st->right_clv >= g.nodes) return fail(PLLGPU_EINVAL, "sumtable references a CLV out of range");
  if (!c->pending.empty() && (clv_is_pending(c, st->right_clv) || (!st->left_is_tip && clv_is_pending(c, st->left_clv))))
    if (int rc = materialise_pending(c)) return rc;
  if (int rc = sumtable_slot(c, slot)) return rc;
  OpPack pack;
  DevOp &d = pack.ops[0];
  memset(&d, 0, sizeof d);
  d.parent = c->sumtable[slot].p;
  d.entries = g.sites_alloc; // with ascertainment bias the per-state extra entries belong to the table
  if (st->left_is_tip)
  {
    if (st->left_clv >= g.tips || !c->tipchars[st->left_clv].p) return fail(PLLGPU_EINVAL, "tip %u has no codes on the device", st->left_clv);
    d.ltip = c->tipchars[st->left_clv].p;
  }
  else
  {
    if (!c->clv[st->left_clv].p) return fail(PLLGPU_EINVAL, "CLV %u unavailable on the device", st->left_clv);
    d.left = c->clv[st->left_clv].p;
  }
  if (!c->clv[st->right_clv].p) return fail(PLLGPU_EINVAL, "CLV %u unavailable on the device", st->right_clv);
  d.right = c->clv[st->right_clv].p;
  d.lmat = c->pmat.p + (size_t)g.prob_matrices * c->pm_stride;
  d.rmat = c->pmat.p + (size_t)(g.prob_matrices + 1) * c->pm_stride;
  d.layout = ((!st->left_is_tip && c->clv_aos[st->left_clv]) ? kAosLeft : 0u) | (c->clv_aos[st->right_clv] ? kAosRight : 0u);
  if (d.layout && !st->gather) return fail(PLLGPU_EINVAL, "a class-compressed CLV met a sumtable without the gather flag");
  if (st->gather)
  {
    d.lsid = c->ids[st->left_clv] ? wide_map(c, st->left_clv) : nullptr;
    d.rsid = c->ids[st->right_clv] ? wide_map(c, st->right_clv) : nullptr;
  }
  const unsigned kind = st->left_is_tip ? 1u : 0u;
  if (int rc = launch_partials(c, pack, 1, g.sites_alloc, kind, st->gather != 0)) return rc;
  if (g.per_rate_scalers && (st->left_scaler >= 0 || st->right_scaler >= 0))
  {
    DevExcess e;
    memset(&e, 0, sizeof e);
    e.table = c->sumtable[slot].p;
    if (int rc = scaler_ptr(c, st->left_is_tip ? -1 : st->left_scaler, e.pscaler)) return rc;
    if (int rc = scaler_ptr(c, st->right_scaler, e.cscaler)) return rc;
    e.psid = d.lsid;
    e.csid = d.rsid;
    e.sites = g.sites_alloc;
    const unsigned tiles = (g.sites_alloc + 63) / 64;
    hipLaunchKernelGGL(k_sumtable_excess, dim3((tiles + 3) / 4), dim3(256), 0, c->stream, e, c->gg);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int pllgpu_sumtable_upload(pllgpu_ctx_t *c, unsigned slot, const double *host)
{
  CHECK_CTX(c);
  if (int rc = sumtable_slot(c, slot)) return rc;
  const size_t n = (size_t)c->geo.sites_alloc * c->span;
  if (int rc = c->scratch.ensure(n)) return rc;
  HIP_TRY(hipMemcpyAsync(c->scratch.p, host, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_aos_to_tiled, dim3(1024), dim3(256), 0, c->stream, c->scratch.p, c->sumtable[slot].p, c->geo.sites_alloc,
                     c->gg.S, c->gg.SP, c->gg.R);
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int pllgpu_sumtable_download(pllgpu_ctx_t *c, unsigned slot, double *host)
{
  CHECK_CTX(c);
  if (slot >= PLLGPU_SUMTABLE_SLOTS || !c->sumtable[slot].p) return fail(PLLGPU_EINVAL, "sumtable slot %u is empty", slot);
  const size_t n = (size_t)c->geo.sites_alloc * c->span;
  if (int rc = c->scratch.ensure(n)) return rc;
  hipLaunchKernelGGL(k_tiled_to_aos, dim3(1024), dim3(256), 0, c->stream, c->sumtable[slot].p, c->scratch.p, c->geo.sites_alloc,
                     c->gg.S, c->gg.SP, c->gg.R);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(host, c->scratch.p, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int pllgpu_sumtable_release(pllgpu_ctx_t *c, unsigned slot)
{
  CHECK_CTX(c);
  if (slot >= PLLGPU_SUMTABLE_SLOTS) return fail(PLLGPU_EINVAL, "sumtable slot %u out of range", slot);
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->sumtable[slot].release();
  return 0;
}

// what one derivative evaluation launches with, for the per-call path and the Newton chain alike
struct DerivLaunch
{
  DevDiag dg;
  DevDeriv dv;
  size_t diag_bytes;
  unsigned local_diag, tpw, blocks;
};

static int deriv_launch_setup(pllgpu_ctx *c, unsigned slot, const unsigned *params_indices, unsigned eval_sites, DerivLaunch &l)
{
  const pllgpu_geometry_t &g = c->geo;
  if (slot >= PLLGPU_SUMTABLE_SLOTS || !c->sumtable[slot].p) return fail(PLLGPU_EINVAL, "sumtable slot %u is empty", slot);
  if (eval_sites == 0 || eval_sites > g.sites_alloc) return fail(PLLGPU_EINVAL, "eval_sites %u out of range", eval_sites);
  if (!c->eigenvals.p || !c->rates.p) return fail(PLLGPU_EINVAL, "eigenvalues / category rates were not uploaded");
  if (int rc = c->diag.ensure((size_t)g.rate_cats * g.states * 4)) return rc;
  DevDiag &dg = l.dg;
  DevDeriv &dv = l.dv;
  memset(&dg, 0, sizeof dg);
  memset(&dv, 0, sizeof dv);
  for (unsigned k = 0; k < g.rate_cats; ++k)
  {
    if (params_indices[k] >= g.rate_matrices) return fail(PLLGPU_EINVAL, "params_indices[%u] out of range", k);
    dg.fidx[k] = dv.fidx[k] = (unsigned char)params_indices[k];
  }
  dg.diag = c->diag.p;
  dg.eigenvals = c->eigenvals.p;
  dg.rates = c->rates.p;
  dg.prop_invar = c->prop_invar.p;
  dg.S = g.states;
  dg.SP = g.states_padded;
  dg.R = g.rate_cats;
  // small tables are formed inside k_derivatives (one launch per evaluation); large ones keep the pre-kernel
  l.diag_bytes = (size_t)g.rate_cats * g.states * 4 * sizeof(double);
  l.local_diag = l.diag_bytes <= 32768 ? 1u : 0u;

  dv.table = c->sumtable[slot].p;
  dv.diag = c->diag.p;
  dv.freqs = c->freqs.p;
  dv.rate_weights = c->rate_weights.p;
  dv.prop_invar = c->prop_invar.p;
  dv.pattern_weights = c->pattern_weights.p;
  dv.invariant = (c->invariant_set && eval_sites <= g.sites) ? c->invariant.p : nullptr;
  dv.block_sums = c->block_sums.p;
  dv.counter = c->counter.p;
  dv.result = c->result_dev;
  dv.sites = eval_sites;
  dv.fenced = c->fenced;
  const unsigned tiles = (eval_sites + 63) / 64;
  l.tpw = (tiles + 4 * 1024 - 1) / (4 * 1024);
  l.blocks = (tiles + 4 * l.tpw - 1) / (4 * l.tpw);
  return 0;
}

// the next sequence word, for a kernel to leave in result[1]
static double next_sequence(pllgpu_ctx *c)
{
  c->seq += 1.0;
  return c->seq;
}

extern "C" int pllgpu_likelihood_derivatives(pllgpu_ctx_t *c, unsigned slot, double branch_length,
                                             const unsigned *params_indices, unsigned eval_sites, double *d_f, double *dd_f)
{
  CHECK_CTX_KEEP_PENDING(c); // (reads the sumtable, no CLV)
  DerivLaunch l;
  if (int rc = deriv_launch_setup(c, slot, params_indices, eval_sites, l)) return rc;
  l.dg.branch_length = branch_length;
  if (!l.local_diag) hipLaunchKernelGGL(k_diagtable, dim3(1), dim3(256), 0, c->stream, l.dg);
  l.dv.sequence = next_sequence(c);
  hipLaunchKernelGGL(k_derivatives, dim3(l.blocks), dim3(256), l.local_diag ? l.diag_bytes : 0, c->stream, l.dv, c->gg, l.tpw, l.dg,
                     l.local_diag);
  HIP_TRY(hipGetLastError());
  if (int rc = wait_for_sequence(c, l.dv.sequence)) return rc;
  *d_f = c->result_host[0];
  *dd_f = c->result_host[2];
  return 0;
}

// Newton's iteration on the device (kernels_deriv.h): one k_derivatives_newton launch per evaluation (behind a
// k_diagtable_newton where the diag table is large), newton_batch = 8 evaluations enqueued at a time with no wait between
// them; behind each batch k_newton_publish and ONE poll. Launches behind the terminal one return at once.
static_assert(kNewtonTraceOut + 3 * PLLGPU_NEWTON_MAX_ITERS <= kResultBytes / sizeof(double), "the trace fits the mapped result block");
static_assert(sizeof(NewtonState) == 8 * sizeof(double), "the state record: eight words in front of the trace");

extern "C" int pllgpu_optimize_branch_length(pllgpu_ctx_t *c, unsigned slot, const unsigned *params_indices, unsigned eval_sites,
                                             const pllgpu_newton_t *opt, pllgpu_newton_result_t *result, double *trace)
{
  CHECK_CTX_KEEP_PENDING(c); // (reads the sumtable, no CLV; the matrix it may write: below)
  const pllgpu_geometry_t &g = c->geo;
  if (!opt || !result) return fail(PLLGPU_EINVAL, "null options / result");
  if (!(opt->t_min >= 0) || !(opt->t_min <= opt->t_max) || !std::isfinite(opt->t_max) || !std::isfinite(opt->t_start) ||
      !(opt->tolerance > 0) || opt->max_iters < 1 || opt->max_iters > PLLGPU_NEWTON_MAX_ITERS || opt->matrix_index < -1 ||
      opt->matrix_index >= (int)g.prob_matrices)
    return fail(PLLGPU_EINVAL, "Newton options out of range");
  const bool with_matrix = opt->matrix_index >= 0;
  if (with_matrix && (!c->evecs.p || !c->ievecs.p)) return fail(PLLGPU_EINVAL, "eigensystem was not uploaded");
  if (with_matrix)
  {
    // the matrix formed at the end is a change like any other: pending CLVs that read it keep the old one aside first
    const unsigned m = (unsigned)opt->matrix_index;
    if (int rc = matrices_change(c, &m, 0, 1)) return rc;
  }
  DerivLaunch l;
  if (int rc = deriv_launch_setup(c, slot, params_indices, eval_sites, l)) return rc;
  if (int rc = c->newton.ensure(8 + 3 * PLLGPU_NEWTON_MAX_ITERS)) return rc;
  DevNewton n;
  memset(&n, 0, sizeof n);
  n.state = reinterpret_cast<NewtonState *>(c->newton.p);
  n.trace = c->newton.p + 8;
  n.t_first = std::min(std::max(opt->t_start, opt->t_min), opt->t_max);
  n.t_min = opt->t_min;
  n.t_max = opt->t_max;
  n.tolerance = opt->tolerance;
  n.max_iters = opt->max_iters;
  n.matrix = with_matrix ? (unsigned)opt->matrix_index : 0u;
  c->last_launches = 0;
  unsigned waits = 0;
  int status = kNewtonRunning;
  for (unsigned done = 0; done < opt->max_iters && status == kNewtonRunning;)
  {
    const unsigned batch = std::min(c->newton_batch, opt->max_iters - done);
    for (unsigned i = 0; i < batch; ++i, ++done)
    {
      n.first = done == 0 ? 1u : 0u;
      if (!l.local_diag)
      {
        hipLaunchKernelGGL(k_diagtable_newton, dim3(1), dim3(256), 0, c->stream, l.dg, n);
        ++c->last_launches;
      }
      hipLaunchKernelGGL(k_derivatives_newton, dim3(l.blocks), dim3(256), l.local_diag ? l.diag_bytes : 0, c->stream, l.dv, c->gg, l.tpw,
                         l.dg, l.local_diag, n);
      ++c->last_launches;
    }
    const double sequence = next_sequence(c);
    hipLaunchKernelGGL(k_newton_publish, dim3(1), dim3(64), 0, c->stream, n.state, n.trace, c->result_dev, sequence, c->fenced);
    ++c->last_launches;
    HIP_TRY(hipGetLastError());
    if (int rc = wait_for_sequence(c, sequence)) return rc;
    ++waits;
    status = (int)c->result_host[kNewtonOut + 3];
  }
  const unsigned iterations = (unsigned)c->result_host[kNewtonOut + 4];
  if (status == kNewtonRunning || iterations < 1 || iterations > opt->max_iters)
    return fail(PLLGPU_ERUNTIME, "the Newton chain ended without a terminal status (status %d after %u evaluations)", status, iterations);
  if (with_matrix)
  {
    // P(result.t) straight from the state record: no value of t crosses to the host and back
    DevPmat d;
    memset(&d, 0, sizeof d);
    memcpy(d.fidx, l.dg.fidx, sizeof d.fidx);
    d.pmat = c->pmat.p;
    d.evecs = c->evecs.p;
    d.ievecs = c->ievecs.p;
    d.evals = c->eigenvals.p;
    d.rates = c->rates.p;
    d.prop_invar = c->prop_invar.p;
    d.mindex = &n.state->matrix;
    d.brlen = &n.state->t;
    d.pm_stride = c->pm_stride;
    d.S = g.states;
    d.SP = g.states_padded;
    d.SPT = c->gg.SPT;
    const size_t lds = (size_t)2 * g.states * (g.states | 1u) * sizeof(double);
    raise_lds_limit((const void *)k_pmatrix, c->device, lds);
    ++c->pm_version[opt->matrix_index];
    hipLaunchKernelGGL(k_pmatrix, dim3(1, g.rate_cats), dim3(256), lds, c->stream, d);
    ++c->last_launches;
    HIP_TRY(hipGetLastError());
  }
  result->t = c->result_host[kNewtonOut + 0];
  result->d_f = c->result_host[kNewtonOut + 1];
  result->dd_f = c->result_host[kNewtonOut + 2];
  result->iterations = iterations;
  result->host_waits = waits;
  result->status = status;
  if (trace) memcpy(trace, c->result_host + kNewtonTraceOut, sizeof(double) * 3 * iterations);
  return 0;
}

// ---- ascertainment-bias terms --------------------------------------------------------------------
extern "C" int pllgpu_asc_terms(pllgpu_ctx_t *c, const pllgpu_edge_t *ed, int is_root, double *terms, unsigned *scalings)
{
  // reads the per-state entries of the edge's two ends and nothing else: pending CLVs are stored first only if an end is one
  // (the correction of the root edge follows every evaluation of an ascertainment-bias partition)
  CHECK_CTX_KEEP_PENDING(c);
  if (int rc = materialise_if_an_end_is_pending(c, ed, is_root != 0)) return rc;
  const pllgpu_geometry_t &g = c->geo;
  if (g.sites_alloc < g.sites + g.states) return fail(PLLGPU_EINVAL, "the partition has no per-state extra entries");
  if (ed->parent_clv >= g.nodes || !c->clv[ed->parent_clv].p) return fail(PLLGPU_EINVAL, "CLV %u unavailable on the device", ed->parent_clv);
  DevAsc a;
  memset(&a, 0, sizeof a);
  a.parent = c->clv[ed->parent_clv].p;
  if (int rc = scaler_ptr(c, ed->parent_scaler, a.pscaler)) return rc;
  if (!is_root)
  {
    if (ed->child_clv >= g.nodes || ed->matrix >= g.prob_matrices) return fail(PLLGPU_EINVAL, "edge references an index out of range");
    if (ed->child_is_tip)
    {
      if (ed->child_clv >= g.tips || !c->tipchars[ed->child_clv].p) return fail(PLLGPU_EINVAL, "tip %u has no codes on the device", ed->child_clv);
      a.ctip = c->tipchars[ed->child_clv].p;
    }
    else
    {
      if (!c->clv[ed->child_clv].p) return fail(PLLGPU_EINVAL, "CLV %u unavailable on the device", ed->child_clv);
      a.child = c->clv[ed->child_clv].p;
      if (int rc = scaler_ptr(c, ed->child_scaler, a.cscaler)) return rc;
    }
    a.mat = c->pmat.p + (size_t)ed->matrix * c->pm_stride;
  }
  for (unsigned k = 0; k < g.rate_cats; ++k)
  {
    if (ed->freqs_indices[k] >= g.rate_matrices) return fail(PLLGPU_EINVAL, "freqs_indices[%u] out of range", k);
    a.fidx[k] = (unsigned char)ed->freqs_indices[k];
  }
  a.freqs = c->freqs.p;
  a.rate_weights = c->rate_weights.p;
  a.out = c->result_dev + kAscOff;
  a.first = g.sites;
  a.per_rate = g.per_rate_scalers ? 1 : 0;
  a.is_root = is_root;
  const unsigned long long *tm = tipmap_ptr(c);
  hipLaunchKernelGGL(k_asc_terms, dim3(g.states), dim3(64), 0, c->stream, a, c->gg, tm);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (unsigned n = 0; n < g.states; ++n)
  {
    terms[n] = c->result_host[kAscOff + n];
    scalings[n] = (unsigned)c->result_host[kAscOff + g.states + n];
  }
  return 0;
}

extern "C" int pllgpu_asc_derivative_terms(pllgpu_ctx_t *c, unsigned slot, int parent_scaler, int child_scaler,
                                           const unsigned *params_indices, double *lk, unsigned *scalings)
{
  CHECK_CTX(c);
  (void)params_indices; // the diag table of the last evaluation already carries them
  const pllgpu_geometry_t &g = c->geo;
  if (g.sites_alloc < g.sites + g.states) return fail(PLLGPU_EINVAL, "the partition has no per-state extra entries");
  if (slot >= PLLGPU_SUMTABLE_SLOTS || !c->sumtable[slot].p || !c->diag.p) return fail(PLLGPU_EINVAL, "no derivative evaluation precedes the ascertainment terms");
  DevAscDeriv a;
  memset(&a, 0, sizeof a);
  a.table = c->sumtable[slot].p;
  a.diag = c->diag.p;
  a.rate_weights = c->rate_weights.p;
  if (int rc = scaler_ptr(c, parent_scaler, a.pscaler)) return rc;
  if (int rc = scaler_ptr(c, child_scaler, a.cscaler)) return rc;
  a.out = c->result_dev + kAscOff;
  a.first = g.sites;
  a.per_rate = g.per_rate_scalers ? 1 : 0;
  hipLaunchKernelGGL(k_asc_deriv_terms, dim3(1), dim3(64), 0, c->stream, a, c->gg);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (unsigned n = 0; n < g.states; ++n)
  {
    lk[3 * n + 0] = c->result_host[kAscOff + 3 * n + 0];
    lk[3 * n + 1] = c->result_host[kAscOff + 3 * n + 1];
    lk[3 * n + 2] = c->result_host[kAscOff + 3 * n + 2];
    scalings[n] = (unsigned)c->result_host[kAscOff + 3 * g.states + n];
  }
  return 0;
}

// ---- transition matrices on the device -----------------------------------------------------------
extern "C" int pllgpu_eigen_upload(pllgpu_ctx_t *c, unsigned index, const double *eigenvecs, const double *inv_eigenvecs,
                                   const double *eigenvals)
{
  CHECK_CTX_KEEP_PENDING(c); // (an input of the matrices formed from here on, of no CLV)
  const pllgpu_geometry_t &g = c->geo;
  if (index >= g.rate_matrices) return fail(PLLGPU_EINVAL, "eigensystem %u out of range", index);
  const size_t n = (size_t)g.states * g.states_padded;
  if (int rc = c->evecs.ensure(n * g.rate_matrices)) return rc;
  if (int rc = c->ievecs.ensure(n * g.rate_matrices)) return rc;
  HIP_TRY(hipMemcpyAsync(c->evecs.p + index * n, eigenvecs, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->ievecs.p + index * n, inv_eigenvecs, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  return pllgpu_eigenvals_upload(c, index, eigenvals);
}

extern "C" int pllgpu_update_pmatrices(pllgpu_ctx_t *c, const unsigned *params_indices, const unsigned *matrix_indices,
                                       const double *branch_lengths, unsigned count)
{
  // like an upload: held work that reads one of these matrices goes out first, pending CLVs that do keep their own copy
  CHECK_CTX_KEEP(c);
  const pllgpu_geometry_t &g = c->geo;
  if (!count) return 0;
  if (!c->evecs.p || !c->ievecs.p || !c->eigenvals.p || !c->rates.p)
    return fail(PLLGPU_EINVAL, "eigensystem / category rates were not uploaded");
  DevPmat d;
  memset(&d, 0, sizeof d);
  for (unsigned k = 0; k < g.rate_cats; ++k)
  {
    if (params_indices[k] >= g.rate_matrices) return fail(PLLGPU_EINVAL, "params_indices[%u] out of range", k);
    d.fidx[k] = (unsigned char)params_indices[k];
  }
  for (unsigned i = 0; i < count; ++i)
    if (matrix_indices[i] >= g.prob_matrices || !(branch_lengths[i] >= 0))
      return fail(PLLGPU_EINVAL, "matrix index %u / branch length %g invalid", matrix_indices[i], branch_lengths[i]);
  if (int rc = matrices_change(c, matrix_indices, 0, count)) return rc;
  for (unsigned i = 0; i < count; ++i) ++c->pm_version[matrix_indices[i]];
  const bool few = count <= kPmatInline;
  if (!few)
  {
    // (a reused staging buffer is overwritten in stream order, behind the launches that still read it)
    if (int rc = c->mindex.ensure(count)) return rc;
    if (int rc = c->brlen.ensure(count)) return rc;
    HIP_TRY(copy_up(c, c->mindex.p, matrix_indices, count * sizeof(unsigned)));
    HIP_TRY(copy_up(c, c->brlen.p, branch_lengths, count * sizeof(double)));
  }
  d.pmat = c->pmat.p;
  d.evecs = c->evecs.p;
  d.ievecs = c->ievecs.p;
  d.evals = c->eigenvals.p;
  d.rates = c->rates.p;
  d.prop_invar = c->prop_invar.p;
  d.mindex = c->mindex.p;
  d.brlen = c->brlen.p;
  d.pm_stride = c->pm_stride;
  d.S = g.states;
  d.SP = g.states_padded;
  d.SPT = c->gg.SPT;
  const size_t lds = (size_t)2 * g.states * (g.states | 1u) * sizeof(double);
  if (few)
  {
    DevPmatFew f;
    f.d = d;
    for (unsigned i = 0; i < count; ++i)
    {
      f.t[i] = branch_lengths[i];
      f.mi[i] = matrix_indices[i];
    }
    raise_lds_limit((const void *)k_pmatrix_few, c->device, lds);
    hipLaunchKernelGGL(k_pmatrix_few, dim3(count, g.rate_cats), dim3(256), lds, c->stream, f);
    HIP_TRY(hipGetLastError());
    return 0;
  }
  raise_lds_limit((const void *)k_pmatrix, c->device, lds);
  for (unsigned first = 0; first < count; first += 65535u) // gridDim.x stays far below its limit; y = rate
  {
    const unsigned nb = std::min(count - first, 65535u);
    DevPmat dd = d;
    dd.mindex += first;
    dd.brlen += first;
    hipLaunchKernelGGL(k_pmatrix, dim3(nb, g.rate_cats), dim3(256), lds, c->stream, dd);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int pllgpu_pmatrix_download(pllgpu_ctx_t *c, unsigned index, double *host)
{
  CHECK_CTX_KEEP_PENDING(c); // (no input of a CLV)
  const pllgpu_geometry_t &g = c->geo;
  if (index >= g.prob_matrices) return fail(PLLGPU_EINVAL, "matrix %u out of range", index);
  HIP_TRY(hipStreamSynchronize(c->stream)); // an earlier upload may still read the staging vector
  c->stage.resize(c->pm_stride);
  HIP_TRY(hipMemcpyAsync(c->stage.data(), c->pmat.p + (size_t)index * c->pm_stride, c->pm_stride * sizeof(double),
                         hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const unsigned S = g.states, SP = g.states_padded, SPT = c->gg.SPT;
  for (unsigned k = 0; k < g.rate_cats; ++k)
    for (unsigned i = 0; i < S; ++i)
    {
      double *row = host + ((size_t)k * S + i) * SP;
      for (unsigned j = 0; j < S; ++j) row[j] = c->stage[((size_t)k * S + j) * SPT + i];
      for (unsigned j = S; j < SP; ++j) row[j] = 0.0;
    }
  return 0;
}

// ---- site-repeats class maps on the device -------------------------------------------------------
extern "C" int pllgpu_repeats_set_ids(pllgpu_ctx_t *c, unsigned node, unsigned ids)
{
  CHECK_CTX(c);
  if (node >= c->geo.nodes) return fail(PLLGPU_EINVAL, "node %u out of range", node);
  if (c->ids[node] != ids)
  {
    ++c->maps_epoch;
    ++c->maps_version;
    ++c->maps_foreign;
  }
  c->ids[node] = ids;
  if (!ids)
  {
    // (the host may settle a parent that cannot be compressed without a class-map call: what such a call leaves behind
    // for an uncompressed parent is left behind here)
    if (c->rep_left[node] != -1 || c->rep_right[node] != -1 || c->map_forms[node] != 0) ++c->maps_epoch;
    c->rep_left[node] = c->rep_right[node] = -1;
    c->map_forms[node] = 0;
    c->map_widened[node] = 0;
  }
  return 0;
}

extern "C" int pllgpu_repeats_download(pllgpu_ctx_t *c, unsigned node, unsigned *site_id, unsigned *id_site, unsigned ids)
{
  CHECK_CTX(c);
  const pllgpu_geometry_t &g = c->geo;
  const unsigned *wide = node < g.nodes ? wide_map(c, node) : nullptr;
  if (!wide || !c->id_site[node].p || ids > g.sites) return fail(PLLGPU_EINVAL, "node %u has no class maps on the device", node);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(site_id, wide, g.sites * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
  if (ids) HIP_TRY(hipMemcpyAsync(id_site, c->id_site[node].p, ids * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

#include "class_map_plan.h"

// ---- fast parsimony (src/fast_parsimony.c): kernels_parsimony.h --------------------------------------------------
// A record of its own, not a pllgpu_ctx: the reference's pll_parsimony_t is independent of the partition it was made
// from, so it owns its stream and ONE device block: [nodes][states][stride] vector words, then the node costs.
// what both kinds of parsimony record (fast: pllgpu_pars, weighted: pllgpu_spars) own to make a call
struct ParsCall
{
  int device = 0;
  hipStream_t stream = nullptr;
  unsigned *args = nullptr;   // per-call arguments and results: accumulators or scores, then ops / pairs
  unsigned char *args_host = nullptr; // pinned: where a call writes its ops / pairs before they are copied up
  size_t args_bytes = 0;
  hipEvent_t args_copied = nullptr;   // the last copy out of args_host has been made
  unsigned last_launches = 0;
};

struct pllgpu_pars : ParsCall
{
  unsigned states = 0, words = 0, stride = 0, nodes = 0;
  unsigned *block = nullptr;  // vectors, then costs
  unsigned *cost = nullptr;   // block + nodes * states * stride
  size_t node_words() const { return (size_t)states * stride; }
};

struct ParsScope // the record's device for the duration of an entry point, the caller's afterwards
{
  int prev = -1, rc = 0;
  explicit ParsScope(const ParsCall *p)
  {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != p->device)
    {
      if (hipSetDevice(p->device) != hipSuccess) rc = fail(PLLGPU_ERUNTIME, "hipSetDevice(%d) failed", p->device);
    }
    else prev = -1;
  }
  ~ParsScope()
  {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};
#define PARS_ENTER(p)                                              \
  if (!(p)) return fail(PLLGPU_EINVAL, "null parsimony record");   \
  ParsScope pars_scope_(p);                                        \
  if (pars_scope_.rc) return pars_scope_.rc

static int pars_args(ParsCall *p, size_t bytes)
{
  if (bytes <= p->args_bytes) return 0;
  HIP_TRY(hipStreamSynchronize(p->stream)); // whatever still reads the old block
  if (p->args) (void)hipFree(p->args);
  if (p->args_host) (void)hipHostFree(p->args_host);
  p->args = nullptr;
  p->args_host = nullptr;
  p->args_bytes = 0;
  bytes = (bytes + 4095) & ~(size_t)4095;
  HIP_TRY(hipMalloc((void **)&p->args, bytes));
  HIP_TRY(hipHostMalloc((void **)&p->args_host, bytes, hipHostMallocDefault));
  p->args_bytes = bytes;
  return 0;
}

// copy `bytes` at args_host + offset to the same offset of the device block, in stream order. The caller has waited for
// args_copied before writing there: a call that returns early (update) leaves its copy in flight
static int pars_args_up(ParsCall *p, size_t offset, size_t bytes)
{
  HIP_TRY(hipMemcpyAsync(reinterpret_cast<unsigned char *>(p->args) + offset, p->args_host + offset, bytes, hipMemcpyHostToDevice, p->stream));
  HIP_TRY(hipEventRecord(p->args_copied, p->stream));
  return 0;
}

// the instantiation that serves a state count (kernels_parsimony.h): fn(SMAX, W, STATES) as integral constants
template <int N>
using pars_int = std::integral_constant<int, N>;
template <class F>
static void pars_variant(unsigned states, F &&fn)
{
  if (states == 4) fn(pars_int<4>(), pars_int<4>(), pars_int<4>());
  else if (states <= 20) fn(pars_int<20>(), pars_int<4>(), pars_int<0>());
  else fn(pars_int<64>(), pars_int<1>(), pars_int<0>());
}

static dim3 pars_grid(const pllgpu_pars *p, unsigned items)
{
  const unsigned w = p->states <= 20 ? 4u : 1u; // pars_variant's W
  const unsigned columns = (p->words + w - 1) / w;
  const unsigned bx = std::min(kParsMaxBlocksX, std::max(1u, (columns + kParsThreads - 1) / kParsThreads));
  return dim3(bx, std::min(items, 32768u), 1);
}

extern "C" pllgpu_pars_t *pllgpu_pars_create(int device, unsigned states, unsigned words, unsigned nodes)
{
  if (states < 2 || states > 64 || nodes == 0 || words >= (1u << 26))
  {
    fail(PLLGPU_EUNSUPPORTED, "parsimony: unsupported shape: states=%u (2..64) words=%u nodes=%u", states, words, nodes);
    return nullptr;
  }
  pllgpu_pars *p = new pllgpu_pars();
  p->device = device;
  p->states = states;
  p->words = words;
  p->stride = (words + 3u) & ~3u;
  p->nodes = nodes;
  ParsScope scope(p);
  const size_t vec_words = (size_t)nodes * p->node_words();
  const size_t bytes = (vec_words + nodes) * sizeof(unsigned);
  bool ok = scope.rc == 0 && hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking) == hipSuccess &&
            hipEventCreateWithFlags(&p->args_copied, hipEventDisableTiming) == hipSuccess && hipMalloc((void **)&p->block, bytes) == hipSuccess;
  // inner vectors and every cost start as zero (the reference leaves inner vectors uninitialised)
  ok = ok && hipMemsetAsync(p->block, 0, bytes, p->stream) == hipSuccess && hipStreamSynchronize(p->stream) == hipSuccess;
  if (!ok)
  {
    fail(PLLGPU_ENOMEM, "parsimony: cannot set up %zu bytes on device %d: %s", bytes, device, hipGetErrorString(hipGetLastError()));
    if (p->block) (void)hipFree(p->block);
    if (p->args_copied) (void)hipEventDestroy(p->args_copied);
    if (p->stream) (void)hipStreamDestroy(p->stream);
    delete p;
    return nullptr;
  }
  p->cost = p->block + vec_words;
  return p;
}

extern "C" void pllgpu_pars_destroy(pllgpu_pars_t *p)
{
  if (!p) return;
  ParsScope scope(p);
  if (p->stream) (void)hipStreamSynchronize(p->stream);
  if (p->args) (void)hipFree(p->args);
  if (p->args_host) (void)hipHostFree(p->args_host);
  if (p->block) (void)hipFree(p->block);
  if (p->args_copied) (void)hipEventDestroy(p->args_copied);
  if (p->stream) (void)hipStreamDestroy(p->stream);
  delete p;
}

extern "C" int pllgpu_pars_upload(pllgpu_pars_t *p, unsigned first, unsigned count, unsigned *const *host)
{
  PARS_ENTER(p);
  if (first + count > p->nodes || first + count < first) return fail(PLLGPU_EINVAL, "parsimony upload: nodes %u+%u of %u", first, count, p->nodes);
  if (!count || !p->words) return 0;
  // one copy for all nodes: the host rows (packedvector_count words) are laid into device rows (stride words)
  std::vector<unsigned> staged((size_t)count * p->node_words(), ~0u);
  for (unsigned n = 0; n < count; ++n)
    for (unsigned s = 0; s < p->states; ++s)
      memcpy(&staged[(size_t)n * p->node_words() + (size_t)s * p->stride], host[first + n] + (size_t)s * p->words, p->words * sizeof(unsigned));
  HIP_TRY(hipMemcpyAsync(p->block + (size_t)first * p->node_words(), staged.data(), staged.size() * sizeof(unsigned), hipMemcpyHostToDevice, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  return 0;
}

extern "C" int pllgpu_pars_download(pllgpu_pars_t *p, unsigned first, unsigned count, unsigned *const *host, unsigned *cost_host)
{
  PARS_ENTER(p);
  if (first + count > p->nodes || first + count < first) return fail(PLLGPU_EINVAL, "parsimony download: nodes %u+%u of %u", first, count, p->nodes);
  if (!count) return 0;
  std::vector<unsigned> staged((size_t)count * p->node_words());
  if (!staged.empty())
    HIP_TRY(hipMemcpyAsync(staged.data(), p->block + (size_t)first * p->node_words(), staged.size() * sizeof(unsigned), hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipMemcpyAsync(cost_host + first, p->cost + first, count * sizeof(unsigned), hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  for (unsigned n = 0; n < count && p->words; ++n)
    for (unsigned s = 0; s < p->states; ++s)
      memcpy(host[first + n] + (size_t)s * p->words, &staged[(size_t)n * p->node_words() + (size_t)s * p->stride], p->words * sizeof(unsigned));
  return 0;
}

extern "C" int pllgpu_pars_update(pllgpu_pars_t *p, const pllgpu_pars_op_t *ops, unsigned count)
{
  PARS_ENTER(p);
  p->last_launches = 0;
  if (!count || !p->words) return 0; // no informative site: every vector is empty and every cost stays 0
  for (unsigned i = 0; i < count; ++i)
    if (ops[i].parent >= p->nodes || ops[i].child1 >= p->nodes || ops[i].child2 >= p->nodes || (i && ops[i].level < ops[i - 1].level))
      return fail(PLLGPU_EINVAL, "parsimony update: op %u out of range or not sorted by level", i);
  // arguments of the call in one block: [count] 64-bit accumulators, then [count] {parent, child1, child2}
  const size_t acc_bytes = (((size_t)count * sizeof(unsigned long long)) + 15) & ~(size_t)15;
  if (int rc = pars_args(p, acc_bytes + (size_t)count * sizeof(ParsOp))) return rc;
  HIP_TRY(hipEventSynchronize(p->args_copied)); // the call before has taken its ops out of args_host (its kernels may still run)
  ParsOp *hops = reinterpret_cast<ParsOp *>(p->args_host + acc_bytes);
  for (unsigned i = 0; i < count; ++i) hops[i] = ParsOp{ops[i].parent, ops[i].child1, ops[i].child2};
  unsigned long long *acc = reinterpret_cast<unsigned long long *>(p->args);
  ParsOp *dops = reinterpret_cast<ParsOp *>(reinterpret_cast<unsigned char *>(p->args) + acc_bytes);
  HIP_TRY(hipMemsetAsync(acc, 0, acc_bytes, p->stream)); // the call's one memset
  if (int rc = pars_args_up(p, acc_bytes, (size_t)count * sizeof(ParsOp))) return rc;
  for (unsigned i = 0; i < count;)
  {
    unsigned j = i;
    while (j < count && ops[j].level == ops[i].level) ++j;
    const dim3 grid = pars_grid(p, j - i);
    pars_variant(p->states, [&](auto smax, auto w, auto fixed) {
      hipLaunchKernelGGL((k_pars_update<decltype(smax)::value, decltype(w)::value, decltype(fixed)::value>), grid, dim3(kParsThreads), 0, p->stream, p->block, p->cost, acc + i, dops + i, j - i,
                         p->states, p->words, p->stride);
    });
    ++p->last_launches;
    i = j;
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

// both score calls: pairs up, one memset, one launch, scores back
template <class Launch>
static int pars_scores(pllgpu_pars *p, const unsigned *pairs, unsigned count, unsigned *scores_host, Launch &&launch)
{
  const size_t score_bytes = (((size_t)count * sizeof(unsigned)) + 15) & ~(size_t)15;
  if (int rc = pars_args(p, score_bytes + (size_t)count * sizeof(ParsPair))) return rc;
  unsigned *scores = p->args;
  ParsPair *dpairs = reinterpret_cast<ParsPair *>(reinterpret_cast<unsigned char *>(p->args) + score_bytes);
  HIP_TRY(hipEventSynchronize(p->args_copied));
  memcpy(p->args_host + score_bytes, pairs, (size_t)count * sizeof(ParsPair));
  HIP_TRY(hipMemsetAsync(scores, 0, score_bytes, p->stream));
  if (int rc = pars_args_up(p, score_bytes, (size_t)count * sizeof(ParsPair))) return rc;
  launch(scores, dpairs);
  p->last_launches = 1;
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(scores_host, scores, (size_t)count * sizeof(unsigned), hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  return 0;
}

static int pars_check_pairs(const pllgpu_pars *p, const unsigned *pairs, unsigned count, const char *who)
{
  for (unsigned i = 0; i < 2u * count; ++i)
    if (pairs[i] >= p->nodes) return fail(PLLGPU_EINVAL, "%s: node %u of %u", who, pairs[i], p->nodes);
  return 0;
}

extern "C" int pllgpu_pars_edge_scores(pllgpu_pars_t *p, const unsigned *pairs, unsigned count, unsigned const_cost, unsigned *scores_host)
{
  PARS_ENTER(p);
  p->last_launches = 0;
  if (!count) return 0;
  if (int rc = pars_check_pairs(p, pairs, count, "parsimony edge scores")) return rc;
  if (!p->words)
  {
    for (unsigned i = 0; i < count; ++i) scores_host[i] = const_cost; // nothing informative: every cost is 0
    return 0;
  }
  return pars_scores(p, pairs, count, scores_host, [&](unsigned *scores, const ParsPair *dpairs) {
    const dim3 grid = pars_grid(p, count);
    pars_variant(p->states, [&](auto smax, auto w, auto fixed) {
      hipLaunchKernelGGL((k_pars_edge_scores<decltype(smax)::value, decltype(w)::value, decltype(fixed)::value>), grid, dim3(kParsThreads), 0, p->stream, p->block, p->cost, dpairs, count, scores,
                         const_cost, p->states, p->words, p->stride);
    });
  });
}

extern "C" int pllgpu_pars_insertion_scores(pllgpu_pars_t *p, unsigned node, const unsigned *edges, unsigned count, unsigned const_cost,
                                            unsigned *scores_host)
{
  PARS_ENTER(p);
  p->last_launches = 0;
  if (node >= p->nodes) return fail(PLLGPU_EINVAL, "parsimony insertion scores: node %u of %u", node, p->nodes);
  if (!count) return 0;
  if (int rc = pars_check_pairs(p, edges, count, "parsimony insertion scores")) return rc;
  if (!p->words)
  {
    for (unsigned i = 0; i < count; ++i) scores_host[i] = const_cost;
    return 0;
  }
  return pars_scores(p, edges, count, scores_host, [&](unsigned *scores, const ParsPair *dedges) {
    const dim3 grid = pars_grid(p, count);
    pars_variant(p->states, [&](auto smax, auto w, auto fixed) {
      hipLaunchKernelGGL((k_pars_insertion_scores<decltype(smax)::value, decltype(w)::value, decltype(fixed)::value>), grid, dim3(kParsThreads), 0, p->stream, p->block, p->cost, node, dedges, count,
                         scores, const_cost, p->states, p->words, p->stride);
    });
  });
}

extern "C" int pllgpu_pars_node_cost(pllgpu_pars_t *p, unsigned node, unsigned *cost_host)
{
  PARS_ENTER(p);
  p->last_launches = 0;
  if (node >= p->nodes) return fail(PLLGPU_EINVAL, "parsimony node cost: node %u of %u", node, p->nodes);
  HIP_TRY(hipMemcpyAsync(cost_host, p->cost + node, sizeof(unsigned), hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  return 0;
}

extern "C" int pllgpu_pars_synchronize(pllgpu_pars_t *p)
{
  PARS_ENTER(p);
  HIP_TRY(hipStreamSynchronize(p->stream));
  return 0;
}

extern "C" unsigned pllgpu_pars_last_launch_count(const pllgpu_pars_t *p) { return p ? p->last_launches : 0; }

// ---- weighted (Sankoff) parsimony (src/parsimony.c): kernels_sankoff.h ---------------------------------------------
// A record like the one above, for a structure made by pll_parsimony_create: every score buffer in the tiled layout
// ([tile][state][64 sites] doubles), every ancestral buffer ([tiles * 64] words), and one block of fixed size: the cost
// matrix with its rows padded to eight doubles, the partial-sum slots, the result word and the tickets of the sums.
constexpr unsigned kSpMaxCands = 4096;   // candidates of one insertion launch: one ticket each
constexpr unsigned kSpMaxSlots = 65536;  // partial sums of one launch
constexpr unsigned kSpScoreBlocks = 1024; // workgroups of a score at most
constexpr unsigned kSpInsBlocks = 64;     // workgroups per insertion candidate at most

struct pllgpu_spars : ParsCall
{
  SpGeo g{};
  unsigned nbuf = 0, nanc = 0;
  int fenced = 0;
  double *buffers = nullptr;
  unsigned *ancestral = nullptr;
  double *fixed = nullptr; // matrix, partials, result, tickets
  double *matrix = nullptr, *partials = nullptr, *result = nullptr;
  unsigned *tickets = nullptr;
  double *stage = nullptr; // buffers in the host mirror's form on their way up or down
  size_t stage_doubles = 0;
  size_t anc_words() const { return (size_t)g.tiles * kSpLanes; }
};

// the instantiation that serves a state count (kernels_sankoff.h): fn(SMAX, NCH) as integral constants
template <class F>
static void sp_variant(unsigned states, F &&fn)
{
  if (states <= 4) fn(pars_int<4>(), pars_int<4>());
  else if (states <= 8) fn(pars_int<8>(), pars_int<8>());
  else if (states <= 24) fn(pars_int<24>(), pars_int<8>());
  else fn(pars_int<64>(), pars_int<8>());
}

static void spars_free(pllgpu_spars *p)
{
  if (p->stream) (void)hipStreamSynchronize(p->stream);
  if (p->args) (void)hipFree(p->args);
  if (p->args_host) (void)hipHostFree(p->args_host);
  if (p->stage) (void)hipFree(p->stage);
  if (p->buffers) (void)hipFree(p->buffers);
  if (p->ancestral) (void)hipFree(p->ancestral);
  if (p->fixed) (void)hipFree(p->fixed);
  if (p->args_copied) (void)hipEventDestroy(p->args_copied);
  if (p->stream) (void)hipStreamDestroy(p->stream);
  delete p;
}

extern "C" pllgpu_spars_t *pllgpu_spars_create(int device, unsigned states, unsigned sites, unsigned buffers, unsigned ancestral_buffers,
                                               const double *matrix)
{
  if (states < 1 || states > 64 || sites == 0 || buffers == 0 || !matrix)
  {
    fail(PLLGPU_EUNSUPPORTED, "weighted parsimony: unsupported shape: states=%u (1..64) sites=%u buffers=%u", states, sites, buffers);
    return nullptr;
  }
  device = pick_device(device);
  if (device < 0) return nullptr;
  pllgpu_spars *p = new pllgpu_spars();
  p->device = device;
  p->g.states = states;
  p->g.sp = (states + 7u) & ~7u;
  p->g.sites = sites;
  p->g.tiles = (sites + kSpLanes - 1) / kSpLanes;
  p->g.buf_doubles = (size_t)p->g.tiles * states * kSpLanes;
  p->nbuf = buffers;
  p->nanc = ancestral_buffers;
  const char *fenced = getenv("PLL_AMD_FENCED_HANDOFF");
  p->fenced = fenced && *fenced && *fenced != '0';
  ParsScope scope(p);
  const size_t matrix_doubles = (size_t)states * p->g.sp;
  const size_t fixed_bytes = (matrix_doubles + kSpMaxSlots + 2) * sizeof(double) + (kSpMaxCands + 2) * sizeof(unsigned);
  const size_t buf_bytes = (size_t)buffers * p->g.buf_doubles * sizeof(double);
  const size_t anc_bytes = (size_t)ancestral_buffers * p->anc_words() * sizeof(unsigned);
  std::vector<double> padded(matrix_doubles, 0.0);
  for (unsigned k = 0; k < states; ++k) memcpy(&padded[(size_t)k * p->g.sp], matrix + (size_t)k * states, states * sizeof(double));
  bool ok = scope.rc == 0 && hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking) == hipSuccess &&
            hipEventCreateWithFlags(&p->args_copied, hipEventDisableTiming) == hipSuccess && hipMalloc((void **)&p->fixed, fixed_bytes) == hipSuccess &&
            hipMalloc((void **)&p->buffers, buf_bytes) == hipSuccess && (!anc_bytes || hipMalloc((void **)&p->ancestral, anc_bytes) == hipSuccess);
  // score buffers, ancestral buffers and every ticket start as zero, as the reference's calloc leaves them
  ok = ok && hipMemsetAsync(p->fixed, 0, fixed_bytes, p->stream) == hipSuccess && hipMemsetAsync(p->buffers, 0, buf_bytes, p->stream) == hipSuccess &&
       (!anc_bytes || hipMemsetAsync(p->ancestral, 0, anc_bytes, p->stream) == hipSuccess) &&
       hipMemcpyAsync(p->fixed, padded.data(), matrix_doubles * sizeof(double), hipMemcpyHostToDevice, p->stream) == hipSuccess &&
       hipStreamSynchronize(p->stream) == hipSuccess;
  if (!ok)
  {
    fail(PLLGPU_ENOMEM, "weighted parsimony: cannot set up %zu bytes on device %d: %s", fixed_bytes + buf_bytes + anc_bytes, device,
         hipGetErrorString(hipGetLastError()));
    spars_free(p);
    return nullptr;
  }
  p->matrix = p->fixed;
  p->partials = p->matrix + matrix_doubles;
  p->result = p->partials + kSpMaxSlots;
  p->tickets = reinterpret_cast<unsigned *>(p->result + 2);
  return p;
}

extern "C" void pllgpu_spars_destroy(pllgpu_spars_t *p)
{
  if (!p) return;
  ParsScope scope(p);
  spars_free(p);
}

static int spars_stage(pllgpu_spars *p, size_t doubles)
{
  if (doubles <= p->stage_doubles) return 0;
  HIP_TRY(hipStreamSynchronize(p->stream));
  if (p->stage) (void)hipFree(p->stage);
  p->stage = nullptr;
  p->stage_doubles = 0;
  HIP_TRY(hipMalloc((void **)&p->stage, doubles * sizeof(double)));
  p->stage_doubles = doubles;
  return 0;
}

// the list of buffers of an upload or a download, on the device
static int spars_index_list(pllgpu_spars *p, const unsigned *indices, unsigned count, const char *who)
{
  for (unsigned i = 0; i < count; ++i)
    if (indices[i] >= p->nbuf) return fail(PLLGPU_EINVAL, "%s: buffer %u of %u", who, indices[i], p->nbuf);
  if (int rc = pars_args(p, (size_t)count * sizeof(unsigned))) return rc;
  HIP_TRY(hipEventSynchronize(p->args_copied));
  memcpy(p->args_host, indices, (size_t)count * sizeof(unsigned));
  return pars_args_up(p, 0, (size_t)count * sizeof(unsigned));
}

extern "C" int pllgpu_spars_upload(pllgpu_spars_t *p, const unsigned *indices, unsigned count, double *const *host)
{
  PARS_ENTER(p);
  if (!count) return 0;
  if (!indices || !host) return fail(PLLGPU_EINVAL, "weighted parsimony upload: null argument");
  const size_t per = (size_t)p->g.sites * p->g.states;
  if (int rc = spars_index_list(p, indices, count, "weighted parsimony upload")) return rc;
  if (int rc = spars_stage(p, (size_t)count * per)) return rc;
  // one copy for all of them; the transposition into tiles happens on the device
  std::vector<double> staged((size_t)count * per);
  for (unsigned i = 0; i < count; ++i) memcpy(&staged[(size_t)i * per], host[indices[i]], per * sizeof(double));
  HIP_TRY(hipMemcpyAsync(p->stage, staged.data(), staged.size() * sizeof(double), hipMemcpyHostToDevice, p->stream));
  for (unsigned first = 0; first < count; first += kSpMaxBlocksY)
    hipLaunchKernelGGL(k_sankoff_upload, dim3(p->g.tiles, std::min(kSpMaxBlocksY, count - first)), dim3(kSpLanes), 0, p->stream, p->buffers,
                       p->stage + (size_t)first * per, p->args + first, p->g);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(p->stream));
  return 0;
}

extern "C" int pllgpu_spars_download(pllgpu_spars_t *p, const unsigned *indices, unsigned count, double *const *host)
{
  PARS_ENTER(p);
  if (!count) return 0;
  if (!indices || !host) return fail(PLLGPU_EINVAL, "weighted parsimony download: null argument");
  const size_t per = (size_t)p->g.sites * p->g.states;
  if (int rc = spars_index_list(p, indices, count, "weighted parsimony download")) return rc;
  if (int rc = spars_stage(p, (size_t)count * per)) return rc;
  for (unsigned first = 0; first < count; first += kSpMaxBlocksY)
    hipLaunchKernelGGL(k_sankoff_download, dim3(p->g.tiles, std::min(kSpMaxBlocksY, count - first)), dim3(kSpLanes), 0, p->stream, p->buffers,
                       p->stage + (size_t)first * per, p->args + first, p->g);
  HIP_TRY(hipGetLastError());
  std::vector<double> staged((size_t)count * per);
  HIP_TRY(hipMemcpyAsync(staged.data(), p->stage, staged.size() * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  for (unsigned i = 0; i < count; ++i) memcpy(host[indices[i]], &staged[(size_t)i * per], per * sizeof(double));
  return 0;
}

extern "C" int pllgpu_spars_download_ancestral(pllgpu_spars_t *p, unsigned first, unsigned count, unsigned *const *host)
{
  PARS_ENTER(p);
  if (first + count > p->nanc || first + count < first) return fail(PLLGPU_EINVAL, "weighted parsimony: ancestral buffers %u+%u of %u", first, count, p->nanc);
  if (!count) return 0;
  // one copy for the whole span; host[i] == NULL: not wanted
  std::vector<unsigned> staged((size_t)count * p->anc_words());
  HIP_TRY(hipMemcpyAsync(staged.data(), p->ancestral + (size_t)first * p->anc_words(), staged.size() * sizeof(unsigned), hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  for (unsigned i = 0; i < count; ++i)
    if (host[first + i]) memcpy(host[first + i], &staged[(size_t)i * p->anc_words()], (size_t)p->g.sites * sizeof(unsigned));
  return 0;
}

// the launch and the 8 bytes back of a score; counts into last_launches
static int spars_score(pllgpu_spars *p, unsigned index, double *score_host)
{
  const unsigned blocks = std::min(p->g.tiles, kSpScoreBlocks);
  hipLaunchKernelGGL(k_sankoff_score, dim3(blocks), dim3(kSpLanes), 0, p->stream, p->buffers, index, p->g, p->partials, p->tickets, p->result, p->fenced);
  ++p->last_launches;
  HIP_TRY(hipGetLastError());
  double score = 0.0;
  HIP_TRY(hipMemcpyAsync(&score, p->result, sizeof(double), hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  *score_host = score;
  return 0;
}

extern "C" int pllgpu_spars_build(pllgpu_spars_t *p, const pllgpu_pars_op_t *ops, unsigned count, unsigned score_index, double *score_host)
{
  PARS_ENTER(p);
  p->last_launches = 0;
  if (!count || !ops || !score_host) return fail(PLLGPU_EINVAL, "weighted parsimony build: empty list or null argument");
  if (score_index >= p->nbuf) return fail(PLLGPU_EINVAL, "weighted parsimony build: buffer %u of %u", score_index, p->nbuf);
  for (unsigned i = 0; i < count; ++i)
    if (ops[i].parent >= p->nbuf || ops[i].child1 >= p->nbuf || ops[i].child2 >= p->nbuf || (i && ops[i].level < ops[i - 1].level))
      return fail(PLLGPU_EINVAL, "weighted parsimony build: op %u out of range or not sorted by level", i);
  if (int rc = pars_args(p, (size_t)count * sizeof(SpOp))) return rc;
  HIP_TRY(hipEventSynchronize(p->args_copied));
  SpOp *hops = reinterpret_cast<SpOp *>(p->args_host);
  for (unsigned i = 0; i < count; ++i) hops[i] = SpOp{ops[i].parent, ops[i].child1, ops[i].child2};
  const SpOp *dops = reinterpret_cast<const SpOp *>(p->args);
  if (int rc = pars_args_up(p, 0, (size_t)count * sizeof(SpOp))) return rc;
  for (unsigned i = 0; i < count;)
  {
    unsigned j = i;
    while (j < count && ops[j].level == ops[i].level) ++j;
    const dim3 grid(p->g.tiles, std::min(j - i, kSpMaxBlocksY));
    sp_variant(p->g.states, [&](auto smax, auto nch) {
      hipLaunchKernelGGL((k_sankoff_build<decltype(smax)::value, decltype(nch)::value>), grid, dim3(kSpLanes), 0, p->stream, p->buffers, p->matrix, dops + i, j - i, p->g);
    });
    ++p->last_launches;
    i = j;
  }
  HIP_TRY(hipGetLastError());
  return spars_score(p, score_index, score_host);
}

extern "C" int pllgpu_spars_score(pllgpu_spars_t *p, unsigned index, double *score_host)
{
  PARS_ENTER(p);
  p->last_launches = 0;
  if (index >= p->nbuf || !score_host) return fail(PLLGPU_EINVAL, "weighted parsimony score: buffer %u of %u", index, p->nbuf);
  return spars_score(p, index, score_host);
}

extern "C" int pllgpu_spars_reconstruct(pllgpu_spars_t *p, const pllgpu_spars_recop_t *ops, unsigned count, const unsigned *tables)
{
  PARS_ENTER(p);
  p->last_launches = 0;
  if (!count) return 0;
  if (!ops || !tables) return fail(PLLGPU_EINVAL, "weighted parsimony reconstruct: null argument");
  for (unsigned i = 0; i < count; ++i)
    if (ops[i].node_score >= p->nbuf || ops[i].parent_score >= p->nbuf || ops[i].node_ancestral >= p->nanc || ops[i].parent_ancestral >= p->nanc ||
        (i && ops[i].level < ops[i - 1].level))
      return fail(PLLGPU_EINVAL, "weighted parsimony reconstruct: op %u out of range or not sorted by level", i);
  for (unsigned i = 0; i < 256; ++i)
    if (tables[256 + i] >= p->g.states) return fail(PLLGPU_EINVAL, "weighted parsimony reconstruct: character %u has state %u of %u", i, tables[256 + i], p->g.states);
  const size_t table_bytes = 512 * sizeof(unsigned);
  if (int rc = pars_args(p, table_bytes + (size_t)count * sizeof(SpRecOp))) return rc;
  HIP_TRY(hipEventSynchronize(p->args_copied));
  memcpy(p->args_host, tables, table_bytes);
  SpRecOp *hops = reinterpret_cast<SpRecOp *>(p->args_host + table_bytes);
  for (unsigned i = 0; i < count; ++i) hops[i] = SpRecOp{ops[i].node_score, ops[i].node_ancestral, ops[i].parent_score, ops[i].parent_ancestral, ops[i].root ? 1u : 0u};
  const SpRecOp *dops = reinterpret_cast<const SpRecOp *>(reinterpret_cast<unsigned char *>(p->args) + table_bytes);
  if (int rc = pars_args_up(p, 0, table_bytes + (size_t)count * sizeof(SpRecOp))) return rc;
  for (unsigned i = 0; i < count;)
  {
    unsigned j = i;
    while (j < count && ops[j].level == ops[i].level) ++j;
    hipLaunchKernelGGL(k_sankoff_reconstruct, dim3(p->g.tiles, std::min(j - i, kSpMaxBlocksY)), dim3(kSpLanes), 0, p->stream, p->buffers, p->ancestral, dops + i, j - i,
                       p->args, p->g);
    ++p->last_launches;
    i = j;
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(p->stream));
  return 0;
}

extern "C" int pllgpu_spars_insertion_scores(pllgpu_spars_t *p, unsigned node, const unsigned *edges, unsigned count, double *scores_host)
{
  PARS_ENTER(p);
  p->last_launches = 0;
  if (node >= p->nbuf) return fail(PLLGPU_EINVAL, "weighted parsimony insertion scores: buffer %u of %u", node, p->nbuf);
  if (!count) return 0;
  if (!edges || !scores_host) return fail(PLLGPU_EINVAL, "weighted parsimony insertion scores: null argument");
  for (unsigned i = 0; i < 2u * count; ++i)
    if (edges[i] >= p->nbuf) return fail(PLLGPU_EINVAL, "weighted parsimony insertion scores: buffer %u of %u", edges[i], p->nbuf);
  // arguments of the call in one block: [count] results, then [count] {a, b}
  const size_t result_bytes = (size_t)count * sizeof(double);
  if (int rc = pars_args(p, result_bytes + (size_t)count * sizeof(SpPair))) return rc;
  HIP_TRY(hipEventSynchronize(p->args_copied));
  memcpy(p->args_host + result_bytes, edges, (size_t)count * sizeof(SpPair));
  double *results = reinterpret_cast<double *>(p->args);
  const SpPair *dedges = reinterpret_cast<const SpPair *>(reinterpret_cast<unsigned char *>(p->args) + result_bytes);
  if (int rc = pars_args_up(p, result_bytes, (size_t)count * sizeof(SpPair))) return rc;
  // the cut of a long list: a launch carries as many candidates as have a ticket and a full set of slots
  const unsigned blocks = std::min(p->g.tiles, kSpInsBlocks);
  const unsigned per_launch = std::min(kSpMaxCands, kSpMaxSlots / blocks);
  for (unsigned first = 0; first < count; first += per_launch)
  {
    const dim3 grid(blocks, std::min(per_launch, count - first));
    sp_variant(p->g.states, [&](auto smax, auto nch) {
      hipLaunchKernelGGL((k_sankoff_insertion<decltype(smax)::value, decltype(nch)::value>), grid, dim3(kSpLanes), 0, p->stream, p->buffers, p->matrix, node, dedges + first, p->g,
                         p->partials, p->tickets, results + first, p->fenced);
    });
    ++p->last_launches;
  }
  HIP_TRY(hipGetLastError());
  // one copy back for all candidates, into memory of our own: the caller's array stays untouched on failure
  std::vector<double> got(count);
  HIP_TRY(hipMemcpyAsync(got.data(), results, result_bytes, hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  memcpy(scores_host, got.data(), result_bytes);
  return 0;
}

extern "C" int pllgpu_spars_synchronize(pllgpu_spars_t *p)
{
  PARS_ENTER(p);
  HIP_TRY(hipStreamSynchronize(p->stream));
  return 0;
}

extern "C" unsigned pllgpu_spars_last_launch_count(const pllgpu_spars_t *p) { return p ? p->last_launches : 0; }

extern "C" void pllgpu_spars_clear_launch_count(pllgpu_spars_t *p)
{
  if (p) p->last_launches = 0;
}
