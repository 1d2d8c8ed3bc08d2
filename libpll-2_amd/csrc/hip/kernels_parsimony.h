// kernels_parsimony.h - bit-parallel Fitch parsimony (reference: src/fast_parsimony.c:405-521, :557-648 and the
// _sse/_avx/_avx2 forms of the same loops) for gfx950.
//
// Layout. A node's vector is state-major as in the reference: `states` rows of 32-bit words, bit b of word w of row s says
// "state s is possible at packed position 32 w + b". On the device a row is `stride` words long, stride = the
// structure's packedvector_count rounded up to four, so that every row starts 16-byte aligned; only the first `words`
// words of a row are ever read or written (a column that straddles the end of a row is loaded and stored word by word,
// the missing words count as all-ones, which is what the reference pads with and adds nothing to any score).
//
// Lanes. A lane owns one column of W consecutive words of EVERY state and keeps both children's columns in registers, so
// the children are streamed from HBM exactly once: the OR over the states of (child1 & child2) has to be complete
// before the first parent word can be formed. Three instantiations, chosen by the state count (pars_variant):
//   states == 4        W = 4 (16-byte loads and stores), the state count is a compile-time constant, 32 data registers;
//   states 2..20       W = 4 (16-byte loads and stores), up to 160 data registers;
//   states 21..64      W = 1, up to 128 data registers - sixteen bytes of 64 states from two children would be 512 registers.
// An operation whose parent is one of its own children is safe: a lane has loaded all it reads before its first store and
// no other lane touches its words.
//
// Costs. The mismatches of a column are counted with __popc, summed over the wave with shuffles, over the workgroup
// through LDS, and leave the workgroup in ONE vector atomic. All sums are integer sums: the result does not depend on the
// order in which waves or workgroups arrive.
//  - update: the atomic is a 64-bit add of {1 << 32 | partial} onto the operation's word of a per-call accumulator
//    (zeroed by the call's one memset). The value it returns tells the workgroup whether it was the last of its
//    operation, and that one - exactly one workgroup per operation - adds the two children's costs and stores the parent's
//    cost. The sum does not land on the parent's cost directly because the parent may be one of the children: its old cost
//    must be read after every partial sum is in and before it is overwritten, and the single atomic orders both without a
//    fence or a second word.
//  - scores: a 32-bit atomicAdd onto scores[pair] (zeroed by the call's memset); the first workgroup of a pair also
//    adds the costs of the nodes involved and const_cost.
// No scalar-memory write of any kind: plain C++ stores and vector atomics.
#pragma once

#include <hip/hip_runtime.h>

constexpr unsigned kParsThreads = 256;
constexpr unsigned kParsMaxBlocksX = 1024; // columns beyond blocks * threads are walked with a grid stride

template <int W>
struct ParsWords
{
  unsigned v[W];
};

// column of W words starting at word w0 of a row of `words` valid words; words beyond the row read as all-ones
template <int W>
__device__ __forceinline__ ParsWords<W> pars_get(const unsigned *row, unsigned w0, unsigned words)
{
  ParsWords<W> r;
  if constexpr (W == 4)
  {
    if (w0 + 4u <= words)
    {
      const uint4 q = *reinterpret_cast<const uint4 *>(row + w0);
      r.v[0] = q.x, r.v[1] = q.y, r.v[2] = q.z, r.v[3] = q.w;
      return r;
    }
  }
#pragma unroll
  for (int k = 0; k < W; ++k) r.v[k] = w0 + k < words ? row[w0 + k] : ~0u;
  return r;
}

template <int W>
__device__ __forceinline__ void pars_put(unsigned *row, unsigned w0, unsigned words, const ParsWords<W> &x)
{
  if constexpr (W == 4)
  {
    if (w0 + 4u <= words)
    {
      *reinterpret_cast<uint4 *>(row + w0) = make_uint4(x.v[0], x.v[1], x.v[2], x.v[3]);
      return;
    }
  }
#pragma unroll
  for (int k = 0; k < W; ++k)
    if (w0 + k < words) row[w0 + k] = x.v[k];
}

// THE Fitch step on one column (src/fast_parsimony.c:574-604). In: the columns of two nodes, row by row. Out:
// both[s] = a & b and any[s] = a | b per state, and the return value `miss`: the positions at which the two nodes share
// no state. The parent's column is both[s] | (miss & any[s]) (fitch_parent); popcount(miss) is what the step adds to a
// score. Callers that only count let the compiler drop the arrays.
template <int SMAX, int W>
__device__ __forceinline__ ParsWords<W> fitch_step(const unsigned *a, const unsigned *b, unsigned states, unsigned stride,
                                                   unsigned w0, unsigned words, ParsWords<W> (&both)[SMAX],
                                                   ParsWords<W> (&any)[SMAX])
{
  ParsWords<W> share;
#pragma unroll
  for (int k = 0; k < W; ++k) share.v[k] = 0u;
#pragma unroll
  for (int s = 0; s < SMAX; ++s)
    if ((unsigned)s < states)
    {
      const ParsWords<W> x = pars_get<W>(a + (size_t)s * stride, w0, words);
      const ParsWords<W> y = pars_get<W>(b + (size_t)s * stride, w0, words);
#pragma unroll
      for (int k = 0; k < W; ++k)
      {
        both[s].v[k] = x.v[k] & y.v[k];
        any[s].v[k] = x.v[k] | y.v[k];
        share.v[k] |= both[s].v[k];
      }
    }
#pragma unroll
  for (int k = 0; k < W; ++k) share.v[k] = ~share.v[k];
  return share;
}

template <int W>
__device__ __forceinline__ ParsWords<W> fitch_parent(const ParsWords<W> &both, const ParsWords<W> &any, const ParsWords<W> &miss)
{
  ParsWords<W> p;
#pragma unroll
  for (int k = 0; k < W; ++k) p.v[k] = both.v[k] | (miss.v[k] & any.v[k]);
  return p;
}

template <int W>
__device__ __forceinline__ unsigned pars_popc(const ParsWords<W> &x)
{
  unsigned n = 0;
#pragma unroll
  for (int k = 0; k < W; ++k) n += __popc(x.v[k]);
  return n;
}

// wave, then workgroup: the total in every lane of wave 0 (only lane 0 of wave 0 uses it)
__device__ __forceinline__ unsigned pars_block_sum(unsigned v)
{
  __shared__ unsigned wave_sums[kParsThreads / 64];
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  const unsigned wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0) wave_sums[wave] = v;
  __syncthreads();
  unsigned total = 0;
  if (wave == 0)
  {
#pragma unroll
    for (unsigned i = 0; i < kParsThreads / 64; ++i) total += wave_sums[i];
  }
  __syncthreads(); // the next operation or pair of a strided block writes wave_sums again
  return total;
}

struct ParsOp
{
  unsigned parent, child1, child2;
};

// pll_fastparsimony_update_vector[_4x4] for every operation of one dependency level: blockIdx.y (strided) = operation,
// blockIdx.x (strided) = columns. STATES > 0: the state count is the constant STATES.
template <int SMAX, int W, int STATES>
__global__ __launch_bounds__(kParsThreads) void k_pars_update(unsigned *vectors, unsigned *cost, unsigned long long *acc,
                                                              const ParsOp *ops, unsigned nops, unsigned states_rt,
                                                              unsigned words, unsigned stride)
{
  const unsigned states = STATES > 0 ? (unsigned)STATES : states_rt;
  const size_t node_words = (size_t)states * stride;
  const unsigned columns = (words + W - 1) / W;
  for (unsigned o = blockIdx.y; o < nops; o += gridDim.y)
  {
    const ParsOp op = ops[o];
    const unsigned *a = vectors + op.child1 * node_words;
    const unsigned *b = vectors + op.child2 * node_words;
    unsigned *p = vectors + op.parent * node_words;
    unsigned mine = 0;
    for (unsigned col = blockIdx.x * kParsThreads + threadIdx.x; col < columns; col += gridDim.x * kParsThreads)
    {
      ParsWords<W> both[SMAX], any[SMAX];
      const unsigned w0 = col * W;
      const ParsWords<W> miss = fitch_step<SMAX, W>(a, b, states, stride, w0, words, both, any);
#pragma unroll
      for (int s = 0; s < SMAX; ++s)
        if ((unsigned)s < states) pars_put<W>(p + (size_t)s * stride, w0, words, fitch_parent<W>(both[s], any[s], miss));
      mine += pars_popc<W>(miss);
    }
    const unsigned total = pars_block_sum(mine);
    if (threadIdx.x == 0)
    {
      // one 64-bit vector atomic per workgroup: arrivals in the high half, the integer sum in the low half (words * 32
      // < 2^32, checked on the host). Whoever sees gridDim.x - 1 earlier arrivals holds the complete sum.
      const unsigned long long before = atomicAdd(&acc[o], (1ull << 32) | total);
      if ((unsigned)(before >> 32) == gridDim.x - 1u)
        cost[op.parent] = (unsigned)before + total + cost[op.child1] + cost[op.child2];
    }
  }
}

struct ParsPair
{
  unsigned a, b;
};

// pll_fastparsimony_edge_score[_4x4] for `npairs` pairs: scores[i] += mismatches(a, b) (+ costs and const_cost once)
template <int SMAX, int W, int STATES>
__global__ __launch_bounds__(kParsThreads) void k_pars_edge_scores(const unsigned *vectors, const unsigned *cost, const ParsPair *pairs,
                                                                   unsigned npairs, unsigned *scores, unsigned const_cost,
                                                                   unsigned states_rt, unsigned words, unsigned stride)
{
  const unsigned states = STATES > 0 ? (unsigned)STATES : states_rt;
  const size_t node_words = (size_t)states * stride;
  const unsigned columns = (words + W - 1) / W;
  for (unsigned i = blockIdx.y; i < npairs; i += gridDim.y)
  {
    const ParsPair pr = pairs[i];
    const unsigned *a = vectors + pr.a * node_words;
    const unsigned *b = vectors + pr.b * node_words;
    unsigned mine = 0;
    for (unsigned col = blockIdx.x * kParsThreads + threadIdx.x; col < columns; col += gridDim.x * kParsThreads)
    {
      ParsWords<W> both[SMAX], any[SMAX];
      mine += pars_popc<W>(fitch_step<SMAX, W>(a, b, states, stride, col * W, words, both, any));
    }
    unsigned total = pars_block_sum(mine);
    if (threadIdx.x == 0)
    {
      if (blockIdx.x == 0) total += cost[pr.a] + cost[pr.b] + const_cost;
      if (total) atomicAdd(&scores[i], total); // integer sum: independent of the order of arrival
    }
  }
}

// Score of the tree obtained by inserting `node` into each of `nedges` edges (a, b): the parent vector F(a, b) of the
// Fitch step is formed in registers, compared with `node` and dropped - what the reference computes with
// pll_fastparsimony_update_vector({tmp, a, b}) followed by pll_fastparsimony_edge_score(tmp, node)
// (src/stepwise.c:507-512). Nothing is written but the scores.
template <int SMAX, int W, int STATES>
__global__ __launch_bounds__(kParsThreads) void k_pars_insertion_scores(const unsigned *vectors, const unsigned *cost, unsigned node,
                                                                        const ParsPair *edges, unsigned nedges, unsigned *scores,
                                                                        unsigned const_cost, unsigned states_rt, unsigned words,
                                                                        unsigned stride)
{
  const unsigned states = STATES > 0 ? (unsigned)STATES : states_rt;
  const size_t node_words = (size_t)states * stride;
  const unsigned columns = (words + W - 1) / W;
  const unsigned *n = vectors + node * node_words;
  for (unsigned i = blockIdx.y; i < nedges; i += gridDim.y)
  {
    const ParsPair e = edges[i];
    const unsigned *a = vectors + e.a * node_words;
    const unsigned *b = vectors + e.b * node_words;
    unsigned mine = 0;
    for (unsigned col = blockIdx.x * kParsThreads + threadIdx.x; col < columns; col += gridDim.x * kParsThreads)
    {
      ParsWords<W> both[SMAX], any[SMAX];
      const unsigned w0 = col * W;
      const ParsWords<W> miss = fitch_step<SMAX, W>(a, b, states, stride, w0, words, both, any);
      ParsWords<W> share;
#pragma unroll
      for (int k = 0; k < W; ++k) share.v[k] = 0u;
#pragma unroll
      for (int s = 0; s < SMAX; ++s)
        if ((unsigned)s < states)
        {
          const ParsWords<W> f = fitch_parent<W>(both[s], any[s], miss);
          const ParsWords<W> x = pars_get<W>(n + (size_t)s * stride, w0, words);
#pragma unroll
          for (int k = 0; k < W; ++k) share.v[k] |= f.v[k] & x.v[k];
        }
#pragma unroll
      for (int k = 0; k < W; ++k) share.v[k] = ~share.v[k];
      mine += pars_popc<W>(miss) + pars_popc<W>(share);
    }
    unsigned total = pars_block_sum(mine);
    if (threadIdx.x == 0)
    {
      if (blockIdx.x == 0) total += cost[e.a] + cost[e.b] + cost[node] + const_cost;
      if (total) atomicAdd(&scores[i], total); // integer sum: independent of the order of arrival
    }
  }
}
