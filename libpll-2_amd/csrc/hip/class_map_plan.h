// class_map_plan.h - part of the pllgpu.hip translation unit: how a site-repeats class-map call is scheduled.
//
// Class maps of a whole op list: every dependency level goes through k_rep_mark + k_rep_assign, the levels back to back,
// and the host reads all class counts once at the end (kernels_repeats.h). What the host must know BEFORE a level's
// counts exist - how large a table slice an op may need - comes from upper bounds: an op's classes are at most its
// cells, its cells at most the product of its children's bounds, and a compressed parent's table is smaller than
// lookup_size by the rule itself.
//
// pllgpu_repeats_classes (at the end) is the sequence of the steps below. Everything that needs no device state comes
// first, for the whole list; class_map_buffers is the one step that may allocate (and so synchronise), and it runs before
// the first launch.
#pragma once

// a call's list, the geometry its kernels share, and what is known of every op before any count exists
struct ClassMapList
{
  const pllgpu_repop_t *ops;
  unsigned count, lookup_size;
  unsigned sites, words;          // bitmap words over the sites
  size_t wstride;                 // ... rounded up to k_rep_scan's rounds
  unsigned bit_ranges, bit_words; // k_rep_bits: 4 ... 32 ranges of the sites per op, each a multiple of 1024 bitmap words (its LDS)
  size_t op_scratch;              // per op of a launch: bitmap, running counts, the ranges' totals and starts
  std::vector<unsigned long long> ub_cells; // per op: the largest table it may have (0: cannot be compressed)
  std::vector<unsigned> ub_classes;         // ... and the most classes
  unsigned long long key;         // FNV-1a over what identifies the list (two lists of one length differ in where compression ends)
};

// the ops of a level, up to kRepOps and kClassMapTableCap cells at a time
struct ClassMapLaunch
{
  unsigned first, n, wgs, mark_lds, assign_lds;
  bool rank; // some op's table may be a large one: k_rep_fold + k_rep_scan + k_rep_rank between k_rep_mark and k_rep_assign
  bool narrow, general; // the builds of k_rep_mark its ops may need (kernels_repeats.h)
  size_t max_cells;     // the largest table an op of the launch may have
  bool fused;           // some op has fused children
  bool assign;          // some op's site -> class pass is k_rep_assign's (not every one deferred to the parent's k_rep_mark)
};

// where a launched op's table and scratch lie, as offsets: the arena and the scratch block may still grow
struct ClassMapPlace
{
  size_t table, bitmap; // cells into rep_table / words into rep_blocksum
  unsigned slice;       // RepOp::slice
};

// the levels up to `ncut` of a list as they go to the device
struct ClassMapPlan
{
  unsigned ncut = 0;
  std::vector<unsigned> fuse;  // per launched op: kRepFuseLeft | kRepFuseRight | kRepDeferred
  std::vector<int> final_slot; // a deferred op's place in rep_final, or -1
  unsigned ndeferred = 0;
  std::vector<ClassMapLaunch> launches;
  std::vector<ClassMapPlace> place;
  size_t arena = 0;            // cells of the largest launch
};

constexpr size_t kClassMapTableCap = (size_t)64 << 20; // cells per launch (256 MB); a single larger op still gets its slice

static inline unsigned long long class_map_child_bound(const ClassMapList &l, int src, unsigned given)
{
  return src >= 0 ? l.ub_classes[src] : given;
}

// The list's checks and upper bounds. Pure: no context state is written and no device buffer is touched.
static int class_map_bounds(const pllgpu_ctx *c, const pllgpu_repop_t *ops, unsigned count, unsigned lookup_size, ClassMapList &l)
{
  const pllgpu_geometry_t &g = c->geo;
  l.ops = ops;
  l.count = count;
  l.lookup_size = lookup_size;
  l.sites = g.sites;
  l.words = (g.sites + 31u) / 32u;
  l.wstride = ((size_t)l.words + kRepScanChunk - 1u) / kRepScanChunk * kRepScanChunk;
  l.bit_ranges = std::max(4u, std::min(kRepBitsMaxRanges, (l.words + 2047u) / 2048u));
  l.bit_words = ((l.words + l.bit_ranges - 1u) / l.bit_ranges + kRepScanThreads - 1u) / kRepScanThreads * kRepScanThreads;
  l.op_scratch = 2u * l.wstride + 2u * kRepBitsMaxRanges;
  l.ub_cells.assign(count, 0ull);
  l.ub_classes.assign(count, 0u);
  l.key = 1469598103934665603ull;
  for (unsigned i = 0; i < count; ++i)
  {
    const pllgpu_repop_t &o = ops[i];
    for (unsigned w : {o.parent, o.left, o.right, o.level}) l.key = (l.key ^ w) * 1099511628211ull;
    if (o.parent >= g.nodes || o.left >= g.nodes || o.right >= g.nodes) return fail(PLLGPU_EINVAL, "repeats op references a node out of range");
    if (i && o.level < ops[i - 1].level) return fail(PLLGPU_EINVAL, "repeats ops are not sorted by level");
    if ((o.lsrc >= 0 && ((unsigned)o.lsrc >= i || ops[o.lsrc].level >= o.level || ops[o.lsrc].parent != o.left)) ||
        (o.rsrc >= 0 && ((unsigned)o.rsrc >= i || ops[o.rsrc].level >= o.level || ops[o.rsrc].parent != o.right)))
      return fail(PLLGPU_EINVAL, "repeats op %u: a child's producer is not an op of a lower level", i);
    unsigned long long cells = class_map_child_bound(l, o.lsrc, o.nleft) * class_map_child_bound(l, o.rsrc, o.nright);
    if (o.force)
    {
      if (o.lsrc >= 0 || o.rsrc >= 0) return fail(PLLGPU_EINVAL, "repeats op %u: a decision taken by the host needs both children's counts", i);
      if (!cells) return fail(PLLGPU_EINVAL, "repeats op: children %u / %u have no class maps on the device", o.left, o.right);
    }
    else if (cells >= lookup_size)
      cells = lookup_size ? lookup_size - 1u : 0u;
    if (cells >= 0x7FFFFFFFull) return fail(PLLGPU_EINVAL, "repeats table of %llu cells exceeds 31-bit addressing", cells);
    l.ub_cells[i] = cells;
    l.ub_classes[i] = (unsigned)std::min<unsigned long long>(cells, l.sites);
  }
  return 0;
}

// How many of the levels to launch. The kernels decide by themselves which parents are compressed, but every level costs
// its launches even when none is; where compression ended the last time this list came is remembered
// (class_map_remember), only the levels up to there are launched, and the rule is evaluated on the host for the ops
// above (class_map_above).
static unsigned class_map_forecast(const pllgpu_ctx *c, const ClassMapList &l)
{
  if (!c->rep_hints || c->rep_hint_count != l.count || c->rep_hint_key != l.key) return l.count;
  unsigned ncut = 0;
  while (ncut < l.count && l.ops[ncut].level <= c->rep_hint_level && c->rep_hint_any) ++ncut;
  return ncut;
}

// ... and the record of where compression ended, for the next call with this list
static void class_map_remember(pllgpu_ctx *c, const ClassMapList &l, const unsigned *counts)
{
  c->rep_hint_count = l.count;
  c->rep_hint_key = l.key;
  c->rep_hint_any = false;
  c->rep_hint_level = 0;
  for (unsigned i = 0; i < l.count; ++i)
    if (counts[i] & kRepFlag)
    {
      c->rep_hint_any = true;
      c->rep_hint_level = std::max(c->rep_hint_level, l.ops[i].level);
    }
}

// A child's site -> class pass inside its parent's k_rep_mark (kernels_repeats.h: kRepFuseLeft): for a child X of the call
// whose table is small for sure, over byte maps, read by exactly one launched op P whose children's maps are both bytes.
// Pure.
static void class_map_fuse(const pllgpu_ctx *c, const ClassMapList &l, ClassMapPlan &plan)
{
  const unsigned ncut = plan.ncut;
  const pllgpu_repop_t *ops = l.ops;
  plan.fuse.assign(ncut, 0u);
  plan.final_slot.assign(ncut, -1);
  plan.ndeferred = 0;
  if (!c->rep_fuse) return;
  std::vector<unsigned> readers(ncut, 0u);
  for (unsigned i = 0; i < ncut; ++i)
  {
    if (ops[i].lsrc >= 0) ++readers[ops[i].lsrc];
    if (ops[i].rsrc >= 0) ++readers[ops[i].rsrc];
  }
  auto bytes = [&](int src, unsigned given) { return class_map_child_bound(l, src, given) <= kRepNarrow; };
  for (unsigned i = 0; i < ncut; ++i)
  {
    const pllgpu_repop_t &o = ops[i];
    if (o.force || !bytes(o.lsrc, o.nleft) || !bytes(o.rsrc, o.nright) || (o.lsrc >= 0 && o.lsrc == o.rsrc)) continue;
    const int kid[2] = {o.lsrc, o.rsrc};
    for (int k = 0; k < 2; ++k)
    {
      const int x = kid[k];
      if (x < 0 || readers[x] != 1u || ops[x].force || !l.ub_cells[x] || l.ub_cells[x] > kRepFuseCells) continue;
      if (!bytes(ops[x].lsrc, ops[x].nleft) || !bytes(ops[x].rsrc, ops[x].nright)) continue;
      plan.fuse[i] |= k ? kRepFuseRight : kRepFuseLeft;
      plan.fuse[x] |= kRepDeferred;
      plan.final_slot[x] = (int)plan.ndeferred++;
    }
  }
}

// The launches: the ops of a level, up to kRepOps and kClassMapTableCap cells at a time, and every op's slice of the arena
// and of the scratch block. Pure.
static void class_map_cut(const pllgpu_ctx *c, const ClassMapList &l, ClassMapPlan &plan)
{
  const unsigned ncut = plan.ncut;
  const pllgpu_repop_t *ops = l.ops;
  plan.launches.clear();
  plan.place.assign(ncut, ClassMapPlace());
  plan.arena = 0;
  for (unsigned done = 0; done < ncut;)
  {
    unsigned room = 0;
    while (done + room < ncut && room < (unsigned)kRepOps && ops[done + room].level == ops[done].level) ++room;
    // workgroups per op: ~512 per launch - all resident at once, and on a 125k-site shard measurably better than 1024
    // (how they split into table parts and site ranges: k_rep_mark)
    const unsigned wgs = c->rep_wgs ? c->rep_wgs : std::max(1u, std::min(64u, (512u + room - 1u) / room));
    ClassMapLaunch L = {done, 0, wgs, kRepSmallCells, 64, false, false, false, 0, false, false};
    size_t cells = 0;
    for (unsigned k = 0; k < room; ++k)
    {
      const unsigned i = done + k;
      const size_t ub = (size_t)l.ub_cells[i];
      // all copies of the table (k_rep_mark): a small one has a copy per workgroup, a large one up to max_ranges - and only
      // while its parts are fewer than the workgroups
      const size_t slice = ((ub <= kRepSmallCells ? ub * wgs : std::max(ub, std::min(ub * c->rep_max_ranges, (size_t)kRepLdsCells * wgs))) + 3u) & ~(size_t)3u;
      if (ub > kRepSmallCells) L.rank = true;
      L.max_cells = std::max(L.max_cells, ub);
      // the narrow build for the ops that are its for sure; an op that only may turn out so goes with the general build
      if (class_map_child_bound(l, ops[i].lsrc, ops[i].nleft) <= kRepNarrow && class_map_child_bound(l, ops[i].rsrc, ops[i].nright) <= kRepNarrow &&
          ub <= kRepSmallCells)
        L.narrow = true;
      else
        L.general = true;
      if (k && cells + slice > kClassMapTableCap) break;
      plan.place[i] = {cells, (size_t)k * l.op_scratch, (unsigned)std::min<size_t>(slice, 0x7FFFFFFFu)};
      if (plan.fuse[i] & (kRepFuseLeft | kRepFuseRight)) L.fused = true;
      if (!(plan.fuse[i] & kRepDeferred) && ub) L.assign = true;
      cells += slice;
      L.mark_lds = std::max<unsigned>(L.mark_lds, (unsigned)std::min<size_t>(ub, kRepLdsCells));
      if (ub <= kRepAssignLds) L.assign_lds = std::max<unsigned>(L.assign_lds, (unsigned)((ub + 3u) & ~(size_t)3u));
      ++L.n;
    }
    plan.arena = std::max(plan.arena, cells);
    plan.launches.push_back(L);
    done += L.n;
  }
}

// Buffers: everything that may allocate (and so synchronise), before the first launch - and the only step that does.
static int class_map_buffers(pllgpu_ctx *c, const ClassMapList &l, const ClassMapPlan &plan)
{
  const size_t melems = map_elems(c);
  for (unsigned i = 0; i < plan.ncut; ++i)
  {
    const pllgpu_repop_t &o = l.ops[i];
    if (!l.ub_cells[i]) continue; // cannot be compressed: nothing to read or write
    // children that come from outside the call: their maps in the form their class count asks for
    const unsigned kid[2] = {o.left, o.right}, kn[2] = {o.nleft, o.nright};
    const int ksrc[2] = {o.lsrc, o.rsrc};
    for (int k = 0; k < 2; ++k)
    {
      if (ksrc[k] >= 0 || !kn[k]) continue;
      if (kn[k] <= kRepNarrow)
      {
        if (int rc = narrow_map(c, kid[k])) return rc;
      }
      else if (!wide_map(c, kid[k]))
        return fail(PLLGPU_EINVAL, "repeats op: child %u has no class maps on the device", kid[k]);
    }
    if (int rc = c->site_id8[o.parent].ensure(melems)) return rc;
    if (l.ub_classes[i] > kRepNarrow)
      if (int rc = c->site_id[o.parent].ensure(melems)) return rc;
    if (int rc = c->id_site[o.parent].ensure(l.ub_classes[i])) return rc;
    if (int rc = c->lent[o.parent].ensure(l.ub_classes[i])) return rc;
    if (int rc = c->rent[o.parent].ensure(l.ub_classes[i])) return rc;
  }
  HIP_TRY(hipGetLastError());
  if (c->rep_fuse)
    if (int rc = c->rep_final.ensure((size_t)std::max(1u, plan.ndeferred) * kRepFuseCells)) return rc;
  for (unsigned i = 0; i < plan.ncut; ++i)
  {
    if (l.ub_cells[i] <= kRepSmallCells) continue;
    // (zeroed when it is new: its last word says whether the rest is what the node's maps derive from)
    DevBuf<unsigned> &kb = c->rep_keep[l.ops[i].parent];
    const size_t had = kb.cap;
    if (int rc = kb.ensure((size_t)l.words + 1u)) return rc;
    if (kb.cap != had) HIP_TRY(hipMemsetAsync(kb.p, 0, kb.cap * sizeof(unsigned), c->stream));
  }
  if (!plan.ncut) return 0;
  if (int rc = c->rep_table.ensure(plan.arena)) return rc;
  // per op of a launch: the bitmap (zero between launches: k_rep_assign clears what k_rep_mark set), then the running counts
  const size_t had = c->rep_blocksum.cap;
  if (int rc = c->rep_blocksum.ensure((size_t)kRepOps * l.op_scratch)) return rc;
  if (c->rep_blocksum.cap != had || c->rep_scratch_dirty) HIP_TRY(hipMemsetAsync(c->rep_blocksum.p, 0, c->rep_blocksum.cap * sizeof(unsigned), c->stream));
  if (c->rep_scratch_dirty) HIP_TRY(hipMemsetAsync(c->rep_sync.p, 0, c->rep_sync.cap * sizeof(unsigned), c->stream));
  c->rep_scratch_dirty = true; // until this call has gone through (class_map_wait)
  if (int rc = c->rep_counts.ensure(l.count)) return rc;
  return c->rep_ops.ensure((size_t)l.count * sizeof(RepOp));
}

// Descriptors up: the offsets of the plan resolved to pointers, now that no buffer moves any more.
static int class_map_descriptors(pllgpu_ctx *c, const ClassMapList &l, const ClassMapPlan &plan)
{
  const unsigned ncut = plan.ncut;
  std::vector<RepOp> &rops = c->rep_ops_host;
  rops.assign(ncut, RepOp());
  for (unsigned i = 0; i < ncut; ++i)
  {
    const pllgpu_repop_t &o = l.ops[i];
    RepOp &r = rops[i];
    r.l8 = c->site_id8[o.left].p;
    r.r8 = c->site_id8[o.right].p;
    r.l32 = c->site_id[o.left].p;
    r.r32 = c->site_id[o.right].p;
    r.p8 = c->site_id8[o.parent].p;
    r.p32 = c->site_id[o.parent].p;
    r.pids = c->id_site[o.parent].p;
    r.lent = c->lent[o.parent].p;
    r.rent = c->rent[o.parent].p;
    r.table = c->rep_table.p + plan.place[i].table;
    r.final = plan.final_slot[i] >= 0 ? c->rep_final.p + (size_t)plan.final_slot[i] * kRepFuseCells : r.table;
    r.keep = l.ub_cells[i] > kRepSmallCells ? c->rep_keep[o.parent].p : nullptr;
    r.bitmap = c->rep_blocksum.p + plan.place[i].bitmap;
    r.lsrc = o.lsrc;
    r.rsrc = o.rsrc;
    r.nleft = o.nleft;
    r.nright = o.nright;
    r.slot = i;
    r.force = o.force ? 1u : 0u;
    r.slice = plan.place[i].slice;
    r.flags = plan.fuse[i];
  }
  // the descriptors go up unless the device array holds exactly these (the same list over the same buffers: the re-evaluation
  // of one tree - a copy of 14 KB is 5 us on the stream, ahead of the first launch)
  if (c->rep_ops_sent.size() == (size_t)ncut * sizeof(RepOp) && c->rep_ops_sent_at == c->rep_ops.p &&
      memcmp(c->rep_ops_sent.data(), rops.data(), c->rep_ops_sent.size()) == 0)
    return 0;
  // (staged in the context's pinned block; ordered behind the previous call's kernels)
  HIP_TRY(copy_up(c, c->rep_ops.p, rops.data(), (size_t)ncut * sizeof(RepOp)));
  c->rep_ops_sent.assign(reinterpret_cast<const unsigned char *>(rops.data()), reinterpret_cast<const unsigned char *>(rops.data() + ncut));
  c->rep_ops_sent_at = c->rep_ops.p;
  return 0;
}

// what every kernel of the call is handed; class_map_launch fills in the launch's own part as it goes
static RepPack class_map_pack(pllgpu_ctx *c, const ClassMapList &l, unsigned ncut)
{
  c->rep_host[c->rep_host_cap + 1u] = 0u;
  RepPack pk;
  memset(&pk, 0, sizeof pk);
  pk.counts = c->rep_counts.p;
  pk.tickets = c->rep_sync.p;
  pk.launch_ticket = c->rep_sync.p + kRepOps;
  pk.changed = c->rep_changed.p;
  pk.all_ops = reinterpret_cast<const RepOp *>(c->rep_ops.p);
  pk.max_ranges = c->rep_max_ranges;
  pk.host_counts = c->rep_host_dev;
  pk.ncounts = ncut;
  pk.host_cap = c->rep_host_cap;
  pk.sites = l.sites;
  pk.lookup = l.lookup_size;
  pk.wstride = (unsigned)l.wstride;
  pk.sequence = ++c->rep_seq;
  pk.fenced = c->fenced;
  return pk;
}

// One launch: the mark builds, fold / bits-or-scan / rank where a table may be large, assign. `pk` is the call's pack: what
// a launch leaves in it is what the next one's kernels see. The call's last kernel that produces counts publishes them.
static void class_map_launch(pllgpu_ctx *c, const ClassMapList &l, const ClassMapLaunch &L, bool last, RepPack &pk)
{
  pk.ops = reinterpret_cast<const RepOp *>(c->rep_ops.p) + L.first;
  pk.nops = L.n;
  pk.mark_wgs = L.wgs;
  pk.mark_lds_cells = L.mark_lds;
  pk.has_rank = L.rank ? 1u : 0u;
  pk.publish = last && !L.rank ? 1u : 0u;
  const unsigned n8 = (L.n + 7u) / 8u * 8u;
  pk.has_narrow = L.narrow ? 1u : 0u;
  pk.has_general = L.general || !L.narrow ? 1u : 0u;
  c->rep_ops_total += L.n;
  c->rep_launches_total += (pk.has_narrow ? 1u : 0u) + (pk.has_general ? 1u : 0u) + (L.rank ? 3u : 0u) + (L.assign ? 1u : 0u);
  if (pk.has_narrow && L.fused)
    hipLaunchKernelGGL(k_rep_mark_narrow_fused, dim3(n8 * L.wgs), dim3(kRepThreads), kRepSmallCells * sizeof(unsigned), c->stream, pk);
  else if (pk.has_narrow)
    hipLaunchKernelGGL(k_rep_mark_narrow, dim3(n8 * L.wgs), dim3(kRepThreads), kRepSmallCells * sizeof(unsigned), c->stream, pk);
  if (pk.has_general)
  {
    const size_t mark_bytes = (size_t)L.mark_lds * sizeof(unsigned);
    raise_lds_limit((const void *)k_rep_mark, c->device, mark_bytes);
    hipLaunchKernelGGL(k_rep_mark, dim3(n8 * L.wgs), dim3(kRepThreads), mark_bytes, c->stream, pk);
  }
  if (L.rank)
  {
    // the bitmap of first sites: in LDS per (op, range of sites) where the tables are small enough for every range's
    // workgroup to read all cells (k_rep_bits), else by atomics in k_rep_fold and one workgroup per op (k_rep_scan)
    const bool bits = c->rep_bits && L.max_cells <= kRepBitsCells;
    pk.bit_ranges = bits ? l.bit_ranges : 0u;
    pk.bit_words = bits ? l.bit_words : 0u;
    hipLaunchKernelGGL(k_rep_fold, dim3(n8 * kRepFoldTiles), dim3(kRepFoldThreads), 0, c->stream, pk);
    pk.publish = last ? 1u : 0u;
    if (bits)
      hipLaunchKernelGGL(k_rep_bits, dim3(n8 * l.bit_ranges), dim3(kRepScanThreads), (size_t)l.bit_words * sizeof(unsigned), c->stream, pk);
    else
      hipLaunchKernelGGL(k_rep_scan, dim3(L.n), dim3(kRepScanThreads), 0, c->stream, pk);
    hipLaunchKernelGGL(k_rep_rank, dim3(n8 * kRepRankTiles), dim3(kRepRankThreads), 0, c->stream, pk);
  }
  // k_rep_assign: a workgroup takes 1..4 rounds of 16384 sites - ~512 workgroups per launch, more rounds where a large
  // table has to be brought into LDS first
  pk.lds_cells = L.assign_lds;
  const size_t assign_bytes = (size_t)L.assign_lds * sizeof(unsigned short);
  const unsigned per_round = kRepAssignThreads * 16u, rounds = (l.sites + per_round - 1u) / per_round;
  pk.assign_iters = std::max(1u, std::min(4u, rounds * L.n / (assign_bytes > 32768 ? 256u : 512u)));
  pk.wgs = (rounds + pk.assign_iters - 1u) / pk.assign_iters;
  raise_lds_limit((const void *)k_rep_assign, c->device, assign_bytes);
  if (L.assign) hipLaunchKernelGGL(k_rep_assign, dim3(n8 * pk.wgs), dim3(kRepAssignThreads), assign_bytes, c->stream, pk);
}

// The class counts arrive in mapped host memory as soon as the last k_rep_mark knows them (its k_rep_assign still runs;
// whatever uses the maps is ordered behind it by the stream): wait for the sequence word, for a bounded time.
static int class_map_wait(pllgpu_ctx *c, unsigned sequence)
{
  const unsigned *seq = c->rep_host + c->rep_host_cap;
  if (int rc = wait_for_word(c, seq, sequence, 50)) return rc;
  if (__atomic_load_n(seq, __ATOMIC_ACQUIRE) != sequence) return fail(PLLGPU_ERUNTIME, "class counts did not arrive");
  if (c->rep_host[c->rep_host_cap + 1u]) return fail(PLLGPU_ERUNTIME, "class maps: a table outgrew what the host had planned for it (%u)", c->rep_host[c->rep_host_cap + 1u]);
  c->rep_scratch_dirty = false;
  return 0;
}

// The ops above the launched levels: the rule (src/repeats.c:100-110), from the counts below them. False if it admits one
// of them after all: the forecast was wrong.
static bool class_map_above(const pllgpu_ctx *c, const ClassMapList &l, unsigned ncut, unsigned *counts_out)
{
  for (unsigned i = 0; i < ncut; ++i) counts_out[i] = c->rep_host[i];
  for (unsigned i = ncut; i < l.count; ++i)
  {
    const pllgpu_repop_t &o = l.ops[i];
    auto ids_of = [&](int src, unsigned given) -> unsigned long long {
      if (src < 0) return given;
      const unsigned w = counts_out[src], n = w & ~kRepFlag;
      return (w & kRepFlag) && n < l.sites ? n : 0u;
    };
    const unsigned long long nl = ids_of(o.lsrc, o.nleft), nr = ids_of(o.rsrc, o.nright), cells = nl * nr;
    if (o.force || (cells && cells < l.lookup_size && nl <= l.sites / 2u && nr <= l.sites / 2u)) return false;
    counts_out[i] = 0u;
  }
  return true;
}

// Adopting the result: which children and which form every parent's maps now have. Cached launches (LevelPlan) carry class
// counts and pointers, not contents: they stay valid when this call found what the last one found - the re-evaluation of
// one tree, again and again, with the reference's pll_update_partials
static int class_map_adopt(pllgpu_ctx *c, const ClassMapList &l, const unsigned *counts)
{
  bool reshaped = false;
  for (unsigned i = 0; i < l.count; ++i)
  {
    const unsigned word = counts[i], classes = word & ~kRepFlag;
    const unsigned parent = l.ops[i].parent;
    if (!(word & kRepFlag))
    {
      reshaped = reshaped || c->rep_left[parent] != -1 || c->rep_right[parent] != -1 || c->map_forms[parent] != 0;
      c->rep_left[parent] = c->rep_right[parent] = -1;
      c->map_forms[parent] = 0;
      c->map_widened[parent] = 0;
      continue;
    }
    if ((unsigned long long)classes > l.ub_cells[i]) return fail(PLLGPU_ERUNTIME, "class maps: op %u reports %u classes of at most %llu", i, classes, l.ub_cells[i]);
    const unsigned char form = classes <= kRepNarrow ? kMap8 : kMap32;
    reshaped = reshaped || c->rep_left[parent] != (int)l.ops[i].left || c->rep_right[parent] != (int)l.ops[i].right || !(c->map_forms[parent] & form);
    c->rep_left[parent] = (int)l.ops[i].left;
    c->rep_right[parent] = (int)l.ops[i].right;
    c->map_forms[parent] = form;
    if (form == kMap8 && c->map_widened[parent])
    {
      // a cached launch reads this node's 32-bit form: bring it up to date behind the bytes
      c->map_widened[parent] = 0;
      if (!wide_map(c, parent)) return fail(PLLGPU_ENOMEM, "class maps: no room for the 32-bit form of node %u", parent);
    }
  }
  if (reshaped) ++c->maps_epoch;
  ++c->maps_version;
  HIP_TRY(hipGetLastError());
  return 0;
}

// the levels up to plan.ncut on the device, their counts on the host
static int class_map_run(pllgpu_ctx *c, const ClassMapList &l, ClassMapPlan &plan)
{
  class_map_fuse(c, l, plan);
  class_map_cut(c, l, plan);
  if (int rc = class_map_buffers(c, l, plan)) return rc;
  if (!plan.ncut) return 0;
  if (int rc = class_map_descriptors(c, l, plan)) return rc;
  RepPack pk = class_map_pack(c, l, plan.ncut);
  for (size_t li = 0; li < plan.launches.size(); ++li) class_map_launch(c, l, plan.launches[li], li + 1 == plan.launches.size(), pk);
  HIP_TRY(hipGetLastError());
  return class_map_wait(c, pk.sequence);
}

extern "C" int pllgpu_repeats_classes(pllgpu_ctx_t *c, const pllgpu_repop_t *ops, unsigned count, unsigned lookup_size, unsigned *counts_out)
{
  CHECK_CTX(c);
  if (!count) return 0;
  if (count > c->rep_host_cap) return fail(PLLGPU_EINVAL, "class maps of %u ops in one call (at most %u)", count, c->rep_host_cap);
  ClassMapList l;
  if (int rc = class_map_bounds(c, ops, count, lookup_size, l)) return rc;
  ++c->rep_calls_total;
  ClassMapPlan plan;
  plan.ncut = class_map_forecast(c, l);
  for (;;)
  {
    if (int rc = class_map_run(c, l, plan)) return rc;
    if (class_map_above(c, l, plan.ncut, counts_out)) break;
    c->rep_hint_count = 0; // the forecast was wrong: every level this time (with every level launched none is left above)
    plan.ncut = count;
  }
  class_map_remember(c, l, counts_out);
  return class_map_adopt(c, l, counts_out);
}
