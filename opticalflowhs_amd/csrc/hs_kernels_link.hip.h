// hs_kernels_link.hip.h -- the regions of frame k linked to those of frame k + 1 by the flow (hs_link_rule.h), where the
// label planes and the flow lie.  Eight kernels, launched one behind the other on one stream; the step is blockIdx.z, step i
// reads its own planes from an argument block by value and owns slice i of the scratch: the rule's table (cells | gone |
// unmatched | over_a, hsln::Table), one count word per 256 cells, and the words the last kernels hand one another (n_links,
// the rows' votes and bests, the columns' bests).  Every word of the scratch that a call reads it has written itself first:
// there is no memset and nothing is carried from one call to the next.
//   k_ln_clear   zeroes the table.
//   k_ln_vote    the hot path.  Grid (ceil(W / 256), rows apportioned as stats_rows does, steps), 256 lanes, a lane per
//                column, the workgroup walks its rows.  Label and flow are loaded coalesced, B's label is gathered, the
//                pixel's word of the table formed (hsln::word_of).  Lanes of a wavefront that share a word issue ONE add of
//                their count (the ballot loop of k_rg_flatten, kLnGroups rounds, lane by lane beyond), and that add goes to
//                LDS: a private copy of the whole table where it fits kLnLdsWords, else an open-addressed table of
//                kLnSlots (word, count) pairs that spills to a global atomic after kLnProbes probes.  Behind the rows the
//                workgroup adds its non-zero words to the global table: two planes of one region each end in ONE global
//                atomic per workgroup, whatever the number of rows and wavefronts.
//   k_ln_count   per 256 cells: the non-zero ones, one word.
//   k_ln_scan    ONE workgroup per step: the exclusive prefix sum of the counts, in place; the total is n_links.
//   k_ln_number  per 256 cells again: the record of every non-zero cell at its rank, below link_capacity.
//   k_ln_rows    a wavefront per row a: votes, non-zero cells and the best b by shuffles; the side_a record.
//   k_ln_cols    a lane per column b, four wavefronts sharing the rows (coalesced across lanes), combined in LDS; side_b.
//   k_ln_finish  ONE workgroup per step: the totals, n_mutual and the result header.
// No atomics behind k_ln_vote, no workgroup waits for another anywhere.  All counts are integers: the outputs do not depend
// on the order of execution.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hs_link_rule.h"

namespace hsk {

constexpr int kLnBatchMax = 8;       // steps per set of launches at most (hs_link.hip.h: fewer where the tables are large)
constexpr int kLnLdsWords = 8192;    // the LDS of a voting workgroup: 32 KiB
constexpr int kLnSlots = 4096;       // ... as a hash: the words in L[0 .. kLnSlots), their counts behind
constexpr int kLnProbes = 8;
constexpr int kLnGroups = 4;         // words of a wavefront that are added by their leaders before the rest goes lane by lane
static_assert(2 * kLnSlots == kLnLdsWords && (kLnSlots & (kLnSlots - 1)) == 0, "words and counts fill the LDS; the slot mask");
static_assert(8 * 256 <= kLnSlots / 2, "a workgroup sees at most 8 rows of 256 pixels: the hash stays at most half full");

// The planes of a set of launches, handed to the kernels by value.
struct LnPlanes {
    const int32_t *a[kLnBatchMax], *b[kLnBatchMax]; // the label planes of frame k and frame k + 1
    const float *u[kLnBatchMax], *v[kLnBatchMax];
    hsln::Link *links[kLnBatchMax];                 // or NULL
    hsln::Side *side_a[kLnBatchMax], *side_b[kLnBatchMax]; // or NULL
    hsln::Result *results[kLnBatchMax];             // or NULL
    long long as, bs, fs;                           // strides in BYTES: labels of a, of b, flow
    int W, H;
    unsigned cap_a, cap_b, link_capacity;
    // the scratch: step i at tab + i * n_tab, counts + i * n_counts, aux + i * n_aux
    uint32_t *tab, *counts, *aux;
    long long n_tab, n_counts, n_aux;
};
static_assert(sizeof(LnPlanes) + 64 <= 1024, "the argument block stays well inside the 4 KiB of kernel arguments");

// aux of a step: n_links, a spare word, the rows' votes, the rows' bests, the columns' bests.
constexpr long long ln_aux_words(unsigned cap_a, unsigned cap_b) { return 2ll + 2ll * cap_a + cap_b; }

#if defined(HS_LINK_KERNELS) // the kernels themselves: hs_link_kernels.hip alone defines it

__device__ __forceinline__ unsigned ln_wave_sum(unsigned v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += (unsigned)__shfl_xor((int)v, d, 64);
    return v;
}

__device__ __forceinline__ unsigned long long ln_wave_sum64(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += (unsigned long long)__shfl_xor((long long)v, d, 64);
    return v;
}

__device__ __forceinline__ unsigned long long ln_wave_max64(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long o = (unsigned long long)__shfl_xor((long long)v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ const float *ln_frow(const float *p, long long stride, int y) { return (const float *)((const uint8_t *)p + (long long)y * stride); }

// Grid: (blocks, 1, steps); 256 lanes, a grid-stride loop over the table's words.
__global__ __launch_bounds__(256) void k_ln_clear(const LnPlanes pl)
{
    const unsigned i = blockIdx.z;
    const uint32_t words = hsln::table_of(pl.cap_a, pl.cap_b).words();
    uint32_t *tab = pl.tab + (long long)i * pl.n_tab;
    for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < words; k += gridDim.x * 256u) tab[k] = 0u;
}

// n more for word w of the workgroup's share: into the private copy, or the hash, or -- the hash full around w's slot --
// the global table itself.
__device__ __forceinline__ void ln_add(uint32_t *L, uint32_t *tab, bool dense, uint32_t w, unsigned n)
{
    if (dense) {
        atomicAdd(L + w, n);
        return;
    }
    const uint32_t h = (w * 2654435761u) >> 20;
#pragma unroll 1
    for (int p = 0; p < kLnProbes; p++) {
        const uint32_t s = (h + (uint32_t)p) & (uint32_t)(kLnSlots - 1);
        const uint32_t old = atomicCAS(L + s, hsln::kNoWord, w);
        if (old == hsln::kNoWord || old == w) {
            atomicAdd(L + kLnSlots + s, n);
            return;
        }
    }
    atomicAdd(tab + w, n);
}

// Grid: (ceil(W / 256), gy, steps); 256 lanes; every lane stays to the end: the wavefront votes together.
__global__ __launch_bounds__(256) void k_ln_vote(const LnPlanes pl)
{
    __shared__ uint32_t L[kLnLdsWords];
    const unsigned i = blockIdx.z;
    const int W = pl.W, H = pl.H;
    const hsln::Table t = hsln::table_of(pl.cap_a, pl.cap_b);
    const uint32_t words = t.words();
    const bool dense = words <= (uint32_t)kLnLdsWords;
    uint32_t *tab = pl.tab + (long long)i * pl.n_tab;
    if (dense) {
        for (uint32_t k = threadIdx.x; k < words; k += 256u) L[k] = 0u;
    } else {
        for (uint32_t k = threadIdx.x; k < (uint32_t)kLnLdsWords; k += 256u) L[k] = k < (uint32_t)kLnSlots ? hsln::kNoWord : 0u;
    }
    __syncthreads();
    const int x = blockIdx.x * 256 + threadIdx.x;
    const unsigned lane = threadIdx.x & 63u;
    const int32_t *A = pl.a[i], *B = pl.b[i];
    const float *U = pl.u[i], *V = pl.v[i];
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        uint32_t w = hsln::kNoWord;
        if (x < W) {
            const int32_t a = hsln::lrow(A, pl.as, y)[x];
            float fu = 0.0f, fv = 0.0f;
            if (a > 0 && (uint32_t)a <= t.cap_a) {
                fu = ln_frow(U, pl.fs, y)[x];
                fv = ln_frow(V, pl.fs, y)[x];
            }
            w = hsln::word_of(t, a, fu, fv, x, y, W, H, B, pl.bs);
        }
        unsigned long long todo = __ballot(w != hsln::kNoWord);
        for (int g = 0; g < kLnGroups && todo; g++) {
            const int lead = __ffsll((long long)todo) - 1;
            const uint32_t lw = (uint32_t)__shfl((int)w, lead, 64);
            const unsigned long long same = __ballot(w == lw);
            if (lane == (unsigned)lead) ln_add(L, tab, dense, lw, (unsigned)__popcll(same));
            todo &= ~same;
        }
        if ((todo >> lane) & 1ull) ln_add(L, tab, dense, w, 1u);
    }
    __syncthreads();
    if (dense) {
        for (uint32_t k = threadIdx.x; k < words; k += 256u) {
            const uint32_t n = L[k];
            if (n) atomicAdd(tab + k, n);
        }
    } else {
        for (uint32_t s = threadIdx.x; s < (uint32_t)kLnSlots; s += 256u) {
            const uint32_t w = L[s];
            if (w != hsln::kNoWord) atomicAdd(tab + w, L[kLnSlots + s]);
        }
    }
}

// Grid: (ceil(cells / 256), 1, steps); 256 lanes, one cell each.
__global__ __launch_bounds__(256) void k_ln_count(const LnPlanes pl)
{
    const unsigned i = blockIdx.z;
    const uint32_t cells = pl.cap_a * pl.cap_b, k = blockIdx.x * 256u + threadIdx.x;
    const uint32_t *tab = pl.tab + (long long)i * pl.n_tab;
    const bool nz = k < cells && tab[k] != 0u;
    __shared__ unsigned part[4];
    const unsigned n = (unsigned)__popcll(__ballot(nz));
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0u) pl.counts[(long long)i * pl.n_counts + blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// Grid: (1, 1, steps); 1024 lanes.  In place: counts[k] becomes the number of non-zero cells in front of block k.
__global__ __launch_bounds__(1024) void k_ln_scan(const LnPlanes pl)
{
    const unsigned i = blockIdx.z;
    uint32_t *counts = pl.counts + (long long)i * pl.n_counts;
    __shared__ unsigned wsum[16];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned carry = 0u;
    for (long long base = 0; base < pl.n_counts; base += 1024) {
        const long long k = base + threadIdx.x;
        const unsigned mine = k < pl.n_counts ? counts[k] : 0u;
        unsigned incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned o = (unsigned)__shfl_up((int)incl, d, 64);
            if (lane >= (unsigned)d) incl += o;
        }
        __syncthreads(); // (the last round's wsum has been read)
        if (lane == 63u) wsum[wave] = incl;
        __syncthreads();
        unsigned before = 0u, total = 0u;
#pragma unroll
        for (int q = 0; q < 16; q++) {
            before += (unsigned)q < wave ? wsum[q] : 0u;
            total += wsum[q];
        }
        if (k < pl.n_counts) counts[k] = carry + before + incl - mine;
        carry += total;
    }
    if (threadIdx.x == 0u) pl.aux[(long long)i * pl.n_aux] = carry;
}

// Grid as k_ln_count.
__global__ __launch_bounds__(256) void k_ln_number(const LnPlanes pl)
{
    const unsigned i = blockIdx.z;
    const uint32_t cells = pl.cap_a * pl.cap_b, k = blockIdx.x * 256u + threadIdx.x;
    const uint32_t *tab = pl.tab + (long long)i * pl.n_tab;
    const uint32_t px = k < cells ? tab[k] : 0u;
    __shared__ unsigned part[4];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long votes = __ballot(px != 0u);
    if (lane == 0u) part[wave] = (unsigned)__popcll(votes);
    __syncthreads();
    hsln::Link *links = pl.links[i];
    if (!links || !px) return;
    unsigned pos = pl.counts[(long long)i * pl.n_counts + blockIdx.x];
    for (unsigned q = 0; q < wave; q++) pos += part[q];
    pos += (unsigned)__popcll(votes & ((1ull << lane) - 1ull));
    if (pos >= pl.link_capacity) return;
    uint32_t *w = (uint32_t *)(links + pos);
    const uint32_t row = k / pl.cap_b;
    w[0] = row + 1u; w[1] = k - row * pl.cap_b + 1u; w[2] = px; w[3] = 0u;
}

// Grid: (ceil(cap_a / 4), 1, steps); 256 lanes, a wavefront per row.
__global__ __launch_bounds__(256) void k_ln_rows(const LnPlanes pl)
{
    const unsigned i = blockIdx.z;
    const uint32_t a = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (a >= pl.cap_a) return; // (the whole wavefront)
    const hsln::Table t = hsln::table_of(pl.cap_a, pl.cap_b);
    const uint32_t *tab = pl.tab + (long long)i * pl.n_tab, *row = tab + (long long)a * pl.cap_b;
    unsigned votes = 0u, n = 0u;
    unsigned long long key = 0ull;
    for (uint32_t b = lane; b < pl.cap_b; b += 64u) {
        const uint32_t px = row[b];
        votes += px;
        n += px != 0u;
        const unsigned long long kb = hsln::best_key(px, b + 1u);
        key = kb > key ? kb : key;
    }
    votes = ln_wave_sum(votes);
    n = ln_wave_sum(n);
    key = ln_wave_max64(key);
    if (lane != 0u) return;
    uint32_t *aux = pl.aux + (long long)i * pl.n_aux + 2;
    aux[a] = votes;
    aux[pl.cap_a + a] = hsln::best_of(key);
    if (pl.side_a[i]) {
        hsln::Side s;
        hsln::fill_side(&s, votes, n, key, tab[t.gone(a + 1u)], tab[t.unmatched(a + 1u)]);
        pl.side_a[i][a] = s;
    }
}

// Grid: (ceil(cap_b / 64), 1, steps); 256 lanes: lane l of wavefront w takes column 64 * blockIdx.x + l over the rows w, w + 4, ...
__global__ __launch_bounds__(256) void k_ln_cols(const LnPlanes pl)
{
    const unsigned i = blockIdx.z;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, b = blockIdx.x * 64u + lane;
    const uint32_t *tab = pl.tab + (long long)i * pl.n_tab;
    __shared__ unsigned spx[4][64], sn[4][64];
    __shared__ unsigned long long skey[4][64];
    unsigned votes = 0u, n = 0u;
    unsigned long long key = 0ull;
    if (b < pl.cap_b)
        for (uint32_t a = wave; a < pl.cap_a; a += 4u) {
            const uint32_t px = tab[(long long)a * pl.cap_b + b];
            votes += px;
            n += px != 0u;
            const unsigned long long ka = hsln::best_key(px, a + 1u);
            key = ka > key ? ka : key;
        }
    spx[wave][lane] = votes; sn[wave][lane] = n; skey[wave][lane] = key;
    __syncthreads();
    if (wave != 0u || b >= pl.cap_b) return;
#pragma unroll
    for (int q = 1; q < 4; q++) {
        votes += spx[q][lane];
        n += sn[q][lane];
        key = skey[q][lane] > key ? skey[q][lane] : key;
    }
    pl.aux[(long long)i * pl.n_aux + 2 + 2ll * pl.cap_a + b] = hsln::best_of(key);
    if (pl.side_b[i]) {
        hsln::Side s;
        hsln::fill_side(&s, votes, n, key, 0u, 0u);
        pl.side_b[i][b] = s;
    }
}

// Grid: (1, 1, steps); 1024 lanes over the rows.
__global__ __launch_bounds__(1024) void k_ln_finish(const LnPlanes pl)
{
    const unsigned i = blockIdx.z;
    const hsln::Table t = hsln::table_of(pl.cap_a, pl.cap_b);
    const uint32_t *tab = pl.tab + (long long)i * pl.n_tab;
    const uint32_t *aux = pl.aux + (long long)i * pl.n_aux;
    const uint32_t *rvotes = aux + 2, *rbest = rvotes + pl.cap_a, *cbest = rbest + pl.cap_a;
    unsigned long long voted = 0ull, gone = 0ull, unmatched = 0ull;
    unsigned mutual = 0u;
    for (uint32_t a = threadIdx.x; a < pl.cap_a; a += 1024u) {
        voted += rvotes[a];
        gone += tab[t.gone(a + 1u)];
        unmatched += tab[t.unmatched(a + 1u)];
        const uint32_t b = rbest[a];
        if (b != 0u && cbest[b - 1u] == a + 1u) mutual++;
    }
    voted = ln_wave_sum64(voted);
    gone = ln_wave_sum64(gone);
    unmatched = ln_wave_sum64(unmatched);
    mutual = ln_wave_sum(mutual);
    __shared__ unsigned long long part[16][3];
    __shared__ unsigned pmut[16];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0u) {
        part[wave][0] = voted; part[wave][1] = gone; part[wave][2] = unmatched;
        pmut[wave] = mutual;
    }
    __syncthreads();
    if (threadIdx.x != 0u || !pl.results[i]) return;
    voted = gone = unmatched = 0ull;
    mutual = 0u;
    for (int q = 0; q < 16; q++) {
        voted += part[q][0]; gone += part[q][1]; unmatched += part[q][2];
        mutual += pmut[q];
    }
    hsln::Result r;
    hsln::finish_result(&r, aux[0], pl.link_capacity, mutual, voted, gone, unmatched, tab[t.over_a()]);
    *pl.results[i] = r;
}

#endif // HS_LINK_KERNELS

// hs_link_kernels.hip: the kernels and their launches, in the order of a call.  vote: the grid of k_ln_vote (stats_rows).
hipError_t launch_link(hipStream_t stream, const LnPlanes &pl, int steps, dim3 vote);

} // namespace hsk
