// hs_radix.hip - everything built on the stable radix partition pass.  In file order:
//
//   partition pass      k_rx_tiles / rx_pass: RxPass, the tile routines (rx_tile, rx_peers, rx_rank, rx_bin_starts, ...) behind
//                       the generic, 4-byte and wide-STRING histogram / scatter kernels
//   fold                GROUP BY's HBM tier: rx_fold_walk (one partition walk) under k_rx_fold (any aggregate) and
//                       k_rx_fold_sum (SUM / COUNT classes), dense output, hs_group_radix_plan / run / emit
//   hs_sort_by_order    the merge order of a multi-rank final aggregate: a stable sort of small integers
//   ORDER BY            hs_order_by: ob_sort and top-k over result rows
//   DISTINCT            hs_distinct: duplicate-row removal over result rows
//   mark-first          hs_mark_first: first-occurrence marks, what COUNT(DISTINCT e) sums
//   windows             hs_window, hs_window_agg, hs_window_nav, hs_window_frames over ob_sort's (partition, order) runs
//   join builds         dense (hs_join_dense_*), keyset (hs_keyset_*: LEFT SEMI / ANTI), hashed (hs_join_hash_*) and STRING
//                       (hs_join_hash_str_*): one partition or window per wave in LDS, jx_count / jx_scan / jx_place / jx_emit
//   join table          hs_join_table_plan / build / count / fill: the routing rule and the table layout of the four join forms
//
// The HBM tier of GROUP BY as a radix partition + on-chip ordered fold (round 2):
//
// Reference loop replaced: AggregateTask over a block, tasks.py:284-310 - a Python dict per block, every row folded
// into its group's accumulators in row order (fp64 / int), written to the shuffle file at the block's end.
//
// Round 1 kept one hash table for all rows in HBM: three passes of random 8-16 B accesses (insert, count, place) over
// a table twice the size of the input, then one lane per group walking its row list - bound by the rate of random
// HBM transactions, ~3 G rows/s.  Here rows are MOVED instead, in streams:
//
//   pass 1, pass 2   stable radix partition of the (key, value...) tuples on hash bits of the key, inside every unit
//                    (file block): histogram per 8192-row tile, one exclusive scan over (segment, bin, tile), scatter.
//                    After the passes every final partition holds <= ~cap/2 rows of ONE unit, still in row order.
//   fold             ONE WAVE per partition: a dictionary + accumulators private to the wave in LDS, rows taken 64 at a
//                    time in order; rows of one step that share a group are ranked (ballots over the slot bits) and
//                    folded in rank order - each group's values are added in ascending row order, i.e. exactly the
//                    reference's sequential fold, bit for bit.  The partition's groups go to a provisional place (the
//                    partition's own start), a scan over the partitions' group counts and a copy make them dense.
//
// Everything is sized on the host from the row count and the largest unit; no host round trip inside
// hs_group_radix_run.  A partition that meets more distinct keys than its dictionary holds raises HS_FLAG_DICT_FULL
// (the caller takes the round-1 path).  Keys: INTEGER / TIMESTAMP (the key word is the value).
#include <algorithm>
#include <type_traits>
#include <utility>
#include "hs_device.h"

#include <cstdlib>
#include <cstring>

extern thread_local char g_hs_err[256];
void hs_set_error(const char* fmt, ...);
extern "C" size_t hs_scan_ws_bytes(int64_t nrows);
extern "C" int hs_exclusive_scan_i64(void* stream, const int64_t* counts, int64_t n, int64_t* start, void* ws);

#define RX_CHECK_LAUNCH(name)                        \
    if (hipGetLastError() != hipSuccess) {           \
        hs_set_error(name ": kernel launch failed"); \
        return HS_E_LAUNCH;                          \
    }

constexpr int RX_THREADS = 1024;               // a partition-pass workgroup
constexpr int RX_PER = 8;                      // rows per thread and tile
constexpr int RX_TILE = RX_THREADS * RX_PER;   // 8192 rows
constexpr int RX_WAVES = RX_THREADS / HS_WAVE;
constexpr int RX_SUB = RX_TILE / RX_WAVES;     // rows of a tile one wave ranks (512, contiguous)
constexpr int RX_MAX_BITS = 8;                 // fan-out of one pass <= 256
constexpr int RX_COLS = 1 + HS_MAX_ACC;        // key + value columns

static_assert(sizeof(hs_radix_plan) % 8 == 0, "hs_radix_plan");

// ---- segments -> tiles ------------------------------------------------------------------------------------------
// tile_base[s] = number of tiles of the segments before s (a tile never straddles two segments)
__global__ void __launch_bounds__(1024) k_rx_tiles(const int64_t* seg_start, int64_t n_seg, int64_t* tile_base) {
    __shared__ int64_t s_part[16];
    const int tid = threadIdx.x, lane = tid & (HS_WAVE - 1), w = tid / HS_WAVE;
    const int64_t per = (n_seg + blockDim.x - 1) / blockDim.x;
    const int64_t s0 = tid * per < n_seg ? tid * per : n_seg, s1 = (s0 + per) < n_seg ? (s0 + per) : n_seg;
    int64_t mine = 0;
    for (int64_t s = s0; s < s1; ++s) mine += (seg_start[s + 1] - seg_start[s] + RX_TILE - 1) / RX_TILE;
    int64_t x = mine;
    for (int d = 1; d < HS_WAVE; d <<= 1) {
        const int64_t t = __shfl_up(x, d, HS_WAVE);
        if (lane >= d) x += t;
    }
    if (lane == HS_WAVE - 1) s_part[w] = x;
    __syncthreads();
    int64_t base = 0, all = 0;
    for (int k = 0; k < (int)(blockDim.x / HS_WAVE); ++k) {
        if (k < w) base += s_part[k];
        all += s_part[k];
    }
    int64_t run = x + base - mine;
    for (int64_t s = s0; s < s1; ++s) {
        tile_base[s] = run;
        run += (seg_start[s + 1] - seg_start[s] + RX_TILE - 1) / RX_TILE;
    }
    if (tid == 0) tile_base[n_seg] = all;
}

// tile -> (segment, tile inside the segment); false past the last tile.  Uniform over the workgroup.
__device__ __forceinline__ bool rx_find_tile(const int64_t* tile_base, int64_t n_seg, int64_t tile, int64_t& seg, int64_t& t) {
    if (tile >= tile_base[n_seg]) return false;
    int64_t lo = 0, hi = n_seg;  // the last s with tile_base[s] <= tile owns it (empty segments share a later base)
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (tile_base[mid] <= tile) lo = mid;
        else hi = mid;
    }
    seg = lo;
    t = tile - tile_base[lo];
    return true;
}

// what a key's bin is cut from: bin = (f(key) >> shift) & (2^bits - 1).  Wave-uniform; every client sets it once.
enum RxBin : int32_t {
    RX_BIN_MIX64 = 0,  // hs_mix64 of the key word (GROUP BY)
    RX_BIN_PLUS1,      // the value + 1 (hs_sort_by_order: -1 sorts first)
    RX_BIN_VALUE,      // the value itself (ob_sort)
    RX_BIN_MIX32,      // rx_mix32 of a 4-byte key: what rx_pass makes of RX_BIN_MIX64 when the 4-byte kernels apply
    RX_BIN_RANGE,      // key - range_bias: partitions are KEY RANGES, most significant bits first (the dense join build)
    RX_BIN_WINDOW,     // the key's hash WINDOW jh_window(key, range_bias) (the hashed join build)
    RX_BIN_WORDS,      // a mix of all the word columns of a wide STRING key (k_rx_histw / k_rx_scatterw: rx_binw)
};

struct RxPass {
    const int64_t* seg_start;  // [n_seg + 1] positions in the row list
    const int64_t* tile_base;  // [n_seg + 1]
    int64_t n_seg;
    int32_t shift, bits;
    int32_t n_cols, first;     // columns that travel (0 = key); first pass reads the key through `key` / `sel`
    int32_t mode, range_bias;  // RxBin and its parameter (RX_BIN_RANGE, RX_BIN_WINDOW: 4-byte keys only)
    int32_t wide;              // a STRING key of one fixed length 8 .. 16 travels as this many 4-byte word columns (2 .. 4), round 3
    hs_col key;
    const int64_t* sel;
    int64_t row0;
    const void* src[RX_COLS];  // position-indexed raw arrays (src[0] unused in the first pass)
    void* dst[RX_COLS];
    int32_t esize[RX_COLS];    // bytes per element: 1, 4 or 8
    int64_t* counters;         // [(tiles) << bits] laid out (segment, bin, tile): counts, then their exclusive scan
};

// the value of column 0 at position i
__device__ __forceinline__ uint64_t rx_key(const RxPass& A, int64_t i) {
    if (A.first) return hs_key_at(A.key, A.sel ? A.sel[i] : A.row0 + i);
    return A.esize[0] == 4 ? (uint64_t)(int64_t)((const int32_t*)A.src[0])[i] : ((const uint64_t*)A.src[0])[i];
}
// 4-byte keys: which partition a key lands in only has to be a function of the key that spreads well - one 32-bit multiply
// and a fold of the high half into the low (the passes take bits 0 .. 15) instead of hs_mix64's 64-bit multiplies, in the
// histogram and the scatter of either pass alike
__device__ __forceinline__ uint32_t rx_mix32(uint32_t k) {
    uint32_t h = k * 0x9E3779B1u;
    h ^= h >> 15;
    h *= 0x85EBCA77u;
    return h ^ (h >> 16);
}
// the hashed join (hs_join_hash_*): a key's window of the table, 0 .. windows - 1 (multiply-shift: no power of two needed)
__device__ __forceinline__ uint32_t jh_window(uint32_t key, uint32_t windows) {
    return (uint32_t)(((uint64_t)rx_mix32(key) * windows) >> 32);
}
// W = uint32_t: the 4-byte kernels, which rx_pass launches in the three 32-bit modes only
template <typename W>
__device__ __forceinline__ uint32_t rx_bin_of(const RxPass& A, W word, int shift, int bits) {
    const uint32_t key = (uint32_t)word, mask = (1u << bits) - 1u;
    switch (A.mode) {
        case RX_BIN_WINDOW: return (jh_window(key, (uint32_t)A.range_bias) >> shift) & mask;
        case RX_BIN_RANGE: return ((key - (uint32_t)A.range_bias) >> shift) & mask;
        case RX_BIN_MIX32: return (rx_mix32(key) >> shift) & mask;
        default:
            if constexpr (sizeof(W) == 8) {
                if (A.mode == RX_BIN_MIX64) return (uint32_t)(hs_mix64(word) >> shift) & mask;
                return (uint32_t)((word + (A.mode == RX_BIN_PLUS1 ? 1u : 0u)) >> shift) & mask;  // RX_BIN_PLUS1, RX_BIN_VALUE
            }
            __builtin_unreachable();
    }
}
__device__ __forceinline__ void rx_move(const void* src, void* dst, int esize, int64_t from, int64_t to) {
    if (esize == 4) ((uint32_t*)dst)[to] = ((const uint32_t*)src)[from];
    else if (esize == 8) ((uint64_t*)dst)[to] = ((const uint64_t*)src)[from];
    else ((uint8_t*)dst)[to] = ((const uint8_t*)src)[from];
}

// ---- the steps every kernel of the pass shares --------------------------------------------------------------------
struct RxTile {
    int64_t b;        // first position of the tile
    int rows;         // 1 .. RX_TILE
    int64_t nt;       // tiles of its segment
    int64_t counter;  // counters[counter + bin * nt]: this tile's cell of a bin
};
// the tile of this workgroup; false past the last tile, for the whole workgroup
__device__ __forceinline__ bool rx_tile(const RxPass& A, RxTile& T) {
    int64_t seg, t;
    if (!rx_find_tile(A.tile_base, A.n_seg, blockIdx.x, seg, t)) return false;
    T.b = A.seg_start[seg] + t * RX_TILE;
    const int64_t left = A.seg_start[seg + 1] - T.b;
    T.rows = left < RX_TILE ? (int)left : RX_TILE;
    T.nt = A.tile_base[seg + 1] - A.tile_base[seg];
    T.counter = (A.tile_base[seg] << A.bits) + t;
    return true;
}
// per-wave counts of the bins (LDS atomics or ranking updates of different waves never meet): zero them - the caller's
// next barrier makes that visible
template <int WAVES>
__device__ __forceinline__ void rx_zero(uint32_t (*hist)[1 << RX_MAX_BITS], int F) {
    for (int i = threadIdx.x; i < WAVES * F; i += WAVES * HS_WAVE) hist[i / F][i % F] = 0;
}
// the tile's histogram: the waves' counts summed into `counters`
template <int WAVES>
__device__ __forceinline__ void rx_hist_store(const RxPass& A, const RxTile& T, const uint32_t (*hist)[1 << RX_MAX_BITS]) {
    __syncthreads();
    const int tid = threadIdx.x;
    if (tid < (1 << A.bits)) {
        uint32_t total = 0;
#pragma unroll
        for (int k = 0; k < WAVES; ++k) total += hist[k][tid];
        A.counters[T.counter + (int64_t)tid * T.nt] = total;
    }
}
// One histogram body: THREADS threads take the tile's keys CHUNK per thread at a time - all loads of a chunk are issued
// before the first count.  load(tile-local row, key) and bin(key) are what the three kernels differ in.
template <int THREADS, int CHUNK, typename Key, typename Load, typename Bin>
__device__ __forceinline__ void rx_hist_tile(const RxPass& A, uint32_t (*hist)[1 << RX_MAX_BITS], Load load, Bin bin) {
    constexpr int WAVES = THREADS / HS_WAVE, PER = RX_TILE / THREADS;
    RxTile T;
    if (!rx_tile(A, T)) return;
    const int tid = threadIdx.x, w = tid / HS_WAVE;
    rx_zero<WAVES>(hist, 1 << A.bits);
    for (int j0 = 0; j0 < PER; j0 += CHUNK) {
        Key key[CHUNK];
#pragma unroll
        for (int j = 0; j < CHUNK; ++j) {
            const int i = tid + (j0 + j) * THREADS;
            if (i < T.rows) load(T, i, key[j]);
            else key[j] = Key{};
        }
        if (j0 == 0) __syncthreads();  // the histograms are zero
#pragma unroll
        for (int j = 0; j < CHUNK; ++j)
            if (tid + (j0 + j) * THREADS < T.rows) atomicAdd(&hist[w][bin(key[j])], 1u);
    }
    rx_hist_store<WAVES>(A, T, hist);
}
// The valid lanes of a 64-row step that hold the same id (a bin, a dictionary slot) as this lane: the AND of one ballot
// per id bit.  Lane order is row order, so a lane's rank among its peers is popc(peers & below).  The partition pass, both
// folds and the join builds' jx_place rank with it; a compile-time `bits` unrolls.
__device__ __forceinline__ uint64_t rx_peers(uint32_t id, bool valid, int bits) {
    uint64_t peers = __ballot(valid);
    for (int bit = 0; bit < bits; ++bit) {
        const bool on = (id >> bit) & 1u;
        const uint64_t bal = __ballot(valid && on);
        peers &= on ? bal : ~bal;
    }
    return peers;
}
// Cross-lane read-after-write through LDS inside ONE wave (the SUM fold's rank rounds and second key word, the join
// builds' cursors and tags): the hardware runs a wave's LDS instructions in order, but the COMPILER must be told not to
// move the plain loads / stores across the hand-over - __builtin_amdgcn_wave_barrier alone is a scheduling barrier, not a
// memory fence.  Wavefront-scope fences cost no instruction (no s_waitcnt at this scope); they pin the order in the source
// instead of in today's codegen.
__device__ __forceinline__ void rx_wave_handover() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// One step of a wave's ranking (64 rows in order): a row's rank among the rows of its bin that this wave has ranked so
// far = the wave's running count of the bin + its rank among this step's equal-bin lanes (rx_peers).  The bin's first
// lane of the step is the only writer of whist_w[bin].
__device__ __forceinline__ uint32_t rx_rank(uint32_t* whist_w, uint32_t bin, bool valid, int bits, uint64_t below) {
    const uint64_t peers = rx_peers(bin, valid, bits);
    const uint32_t prior = valid ? whist_w[bin] : 0u;
    const uint32_t rank = (uint32_t)__popcll(peers & below);
    if (valid && rank == 0) whist_w[bin] = prior + (uint32_t)__popcll(peers);
    return prior + rank;
}
// From the waves' counts (ranking done) to whist[w][bin] = tile-local start of (wave, bin) and gbase[bin] = "global
// position minus tile-local position" of the bin's rows: a scan over the waves per bin, an exclusive scan of the bin
// totals (threads 0 .. 255 = waves 0 .. 3) and the tile's scanned counter.  Barriers at both ends.
__device__ __forceinline__ void rx_bin_starts(const RxPass& A, const RxTile& T, uint32_t (*whist)[1 << RX_MAX_BITS], int64_t* gbase,
                                              uint32_t* s_wave_tot) {
    const int tid = threadIdx.x, lane = tid & (HS_WAVE - 1), w = tid / HS_WAVE, F = 1 << A.bits;
    __syncthreads();
    uint32_t bin_total = 0;
    if (tid < F) {
        uint32_t run = 0;
#pragma unroll
        for (int k = 0; k < RX_WAVES; ++k) {
            const uint32_t c = whist[k][tid];
            whist[k][tid] = run;
            run += c;
        }
        bin_total = run;
        gbase[tid] = A.counters[T.counter + (int64_t)tid * T.nt];
    }
    uint32_t x = bin_total;
    for (int d = 1; d < HS_WAVE; d <<= 1) {
        const uint32_t up = __shfl_up(x, d, HS_WAVE);
        if (lane >= d) x += up;
    }
    if (w < 4 && lane == HS_WAVE - 1) s_wave_tot[w] = x;
    __syncthreads();
    if (tid < F) {
        const uint32_t before = (w > 0 ? s_wave_tot[0] : 0u) + (w > 1 ? s_wave_tot[1] : 0u) + (w > 2 ? s_wave_tot[2] : 0u);
        const uint32_t bin_start = before + x - bin_total;
        gbase[tid] -= bin_start;
#pragma unroll
        for (int k = 0; k < RX_WAVES; ++k) whist[k][tid] += bin_start;
    }
    __syncthreads();
}
// A staged column (the tile in bin order in LDS) leaves by consecutive threads: the rows of a bin (32 on average at
// fan-out 256) go out as one or two contiguous segments instead of one 4-8 B store per row and bin - the store path of
// a CU takes a request per distinct line, not per byte.  The barrier in front: the column is staged.
template <typename E>
__device__ __forceinline__ void rx_write_out(E* dst, const E* stage, const uint8_t* sbin, const int64_t* gbase, int rows) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RX_PER; ++k) {
        const int i = threadIdx.x + k * RX_THREADS;
        if (i < rows) dst[gbase[sbin[i]] + i] = stage[i];
    }
}

__global__ void __launch_bounds__(RX_THREADS) k_rx_hist(const RxPass A_kernarg) {
    HS_KERNARG(RxPass, A);
    __shared__ uint32_t hist[RX_WAVES][1 << RX_MAX_BITS];
    rx_hist_tile<RX_THREADS, RX_PER, uint64_t>(
        A, hist, [&](const RxTile& T, int i, uint64_t& word) { word = rx_key(A, T.b + i); },
        [&](uint64_t word) { return rx_bin_of(A, word, A.shift, A.bits); });
}

// Stable scatter of a tile.  Wave w ranks rows [w * 512, (w + 1) * 512) of the tile, 64 at a time in order (rx_rank); a
// scan over the waves per bin and the tile's scanned counter finish the address (rx_bin_starts).  The tile is first put
// in bin order in LDS, one column at a time, and written out by consecutive threads (rx_write_out).
// two workgroups per CU (<= 64 VGPRs, a few spilled) beat one at 94 VGPRs: 560 us against 840 us per pass of 64 M rows
__global__ void __launch_bounds__(RX_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8))) k_rx_scatter(const RxPass A_kernarg) {
    HS_KERNARG(RxPass, A);
    __shared__ uint32_t whist[RX_WAVES][1 << RX_MAX_BITS];
    __shared__ int64_t gbase[1 << RX_MAX_BITS];
    __shared__ uint32_t s_wave_tot[4];
    extern __shared__ __align__(16) uint8_t rx_stage[];  // sbin[RX_TILE] u8, then stage[RX_TILE] of the widest column
    RxTile T;
    if (!rx_tile(A, T)) return;
    const int tid = threadIdx.x, lane = tid & (HS_WAVE - 1), w = tid / HS_WAVE;
    rx_zero<RX_WAVES>(whist, 1 << A.bits);
    __syncthreads();
    // all loads of a phase are issued before the first dependent use: the kernel would otherwise pay one global
    // round trip per row step (the ranking's LDS updates and the scatter's stores fence the loads behind them)
    uint64_t word[RX_PER];
    uint32_t bin[RX_PER], local[RX_PER];
    const uint64_t below = (1ull << lane) - 1ull;
    const int first = w * RX_SUB + lane;  // tile-local row of step 0
#pragma unroll
    for (int j = 0; j < RX_PER; ++j) {
        const int i = first + j * HS_WAVE;
        word[j] = i < T.rows ? rx_key(A, T.b + i) : 0;
    }
#pragma unroll
    for (int j = 0; j < RX_PER; ++j) {
        const bool valid = first + j * HS_WAVE < T.rows;
        bin[j] = valid ? rx_bin_of(A, word[j], A.shift, A.bits) : 0u;
        local[j] = rx_rank(whist[w], bin[j], valid, A.bits, below);
    }
    rx_bin_starts(A, T, whist, gbase, s_wave_tot);
    uint8_t* sbin = rx_stage;
    uint8_t* stage = rx_stage + RX_TILE;
    uint32_t lpos2[RX_PER / 2];  // two 16-bit tile-local positions per register; 0xffff: no row
#pragma unroll
    for (int j = 0; j < RX_PER; ++j) {
        const bool valid = first + j * HS_WAVE < T.rows;
        const uint32_t at = valid ? whist[w][bin[j]] + local[j] : 0xffffu;
        if (valid) sbin[at] = (uint8_t)bin[j];
        lpos2[j / 2] = (j & 1) ? (lpos2[j / 2] | (at << 16)) : at;
    }
    auto lpos = [&](int j) -> uint32_t { return (lpos2[j / 2] >> ((j & 1) * 16)) & 0xffffu; };
    auto write_out = [&](void* dst, int es) {
        if (es == 4) rx_write_out((uint32_t*)dst, (const uint32_t*)stage, sbin, gbase, T.rows);
        else if (es == 8) rx_write_out((uint64_t*)dst, (const uint64_t*)stage, sbin, gbase, T.rows);
        else rx_write_out((uint8_t*)dst, (const uint8_t*)stage, sbin, gbase, T.rows);
        __syncthreads();  // the column has left the stage
    };
    {   // the key column, from registers
        const int es = A.esize[0];
#pragma unroll
        for (int j = 0; j < RX_PER; ++j) {
            if (lpos(j) == 0xffffu) continue;
            if (es == 4) ((uint32_t*)stage)[lpos(j)] = (uint32_t)word[j];
            else ((uint64_t*)stage)[lpos(j)] = word[j];
        }
        write_out(A.dst[0], es);
    }
    for (int c = 1; c < A.n_cols; ++c) {
        const int es = A.esize[c];
        const void* src = A.src[c];
        uint64_t v[RX_PER];
#pragma unroll
        for (int j = 0; j < RX_PER; ++j) {
            const int64_t i = T.b + first + j * HS_WAVE;
            v[j] = lpos(j) == 0xffffu ? 0 : (es == 4 ? (uint64_t)((const uint32_t*)src)[i] : es == 8 ? ((const uint64_t*)src)[i] : (uint64_t)((const uint8_t*)src)[i]);
        }
#pragma unroll
        for (int j = 0; j < RX_PER; ++j) {
            if (lpos(j) == 0xffffu) continue;
            if (es == 4) ((uint32_t*)stage)[lpos(j)] = (uint32_t)v[j];
            else if (es == 8) ((uint64_t*)stage)[lpos(j)] = v[j];
            else stage[lpos(j)] = (uint8_t)v[j];
        }
        write_out(A.dst[c], es);
    }
}

// ---- the pass for 4-byte tuples (round 3) --------------------------------------------------------------------------
// INTEGER key + up to three 4-byte value columns (f32 / i32: what SUM, AVG, COUNT over stored columns carry): the same
// tile, ranking and staging as k_rx_hist / k_rx_scatter with everything that was decided per element at run time
// (element size, first pass or later, selection, key kind) decided at compile time, the value columns waiting in
// registers, and a 32-bit bin.  FIRST: the key is read from the table's INTEGER column at row0 + position, or through
// the row list behind a WHERE.
template <bool FIRST>
struct Rx4Keys {
    const int32_t* keys;  // at the tile's first position
    const int64_t* sel;
    const int32_t* table;
    __device__ __forceinline__ Rx4Keys(const RxPass& A, const RxTile& T)
        : keys((FIRST ? (const int32_t*)A.key.data + A.row0 : (const int32_t*)A.src[0]) + T.b),
          sel(FIRST && A.sel ? A.sel + T.b : nullptr), table((const int32_t*)A.key.data) {}
    __device__ __forceinline__ uint32_t operator()(int i) const { return (uint32_t)(sel ? table[sel[i]] : keys[i]); }
};

constexpr int RX_H4_THREADS = 256;                   // the histogram of a tile needs no ranking: four waves, 32 keys per lane
constexpr int RX_H4_PER = RX_TILE / RX_H4_THREADS;
template <bool FIRST>
__global__ void __launch_bounds__(RX_H4_THREADS) k_rx_hist4(const RxPass A_kernarg) {
    HS_KERNARG(RxPass, A);
    __shared__ uint32_t hist[RX_H4_THREADS / HS_WAVE][1 << RX_MAX_BITS];
    const int shift = A.shift, bits = A.bits;
    rx_hist_tile<RX_H4_THREADS, RX_H4_PER, uint32_t>(
        A, hist, [&](const RxTile& T, int i, uint32_t& key) { key = Rx4Keys<FIRST>(A, T)(i); },
        [&](uint32_t key) { return rx_bin_of(A, key, shift, bits); });
}

template <int NV, bool FIRST>
__global__ void __launch_bounds__(RX_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8))) k_rx_scatter4(const RxPass A_kernarg) {
    HS_KERNARG(RxPass, A);
    __shared__ uint32_t whist[RX_WAVES][1 << RX_MAX_BITS];
    __shared__ int64_t gbase[1 << RX_MAX_BITS];
    __shared__ uint32_t s_wave_tot[4];
    __shared__ uint8_t sbin[RX_TILE];
    __shared__ uint32_t stage[RX_TILE];
    RxTile T;
    if (!rx_tile(A, T)) return;
    const int tid = threadIdx.x, lane = tid & (HS_WAVE - 1), w = tid / HS_WAVE;
    const int64_t b = T.b;
    const int rows = T.rows;
    constexpr int NVR = NV > 0 ? NV : 1;
    uint32_t key[RX_PER], val[NVR][RX_PER];
    const int first = w * RX_SUB + lane;  // tile-local row of step 0
    const Rx4Keys<FIRST> key_at(A, T);
#pragma unroll
    for (int j = 0; j < RX_PER; ++j) {
        const int i = first + j * HS_WAVE;
        key[j] = i >= rows ? 0u : key_at(i);
    }
#pragma unroll
    for (int c = 0; c < NV; ++c) {
        if (FIRST && A.src[1 + c] == nullptr) {  // (uniform) a first pass without this column: it carries the row's POSITION
#pragma unroll
            for (int j = 0; j < RX_PER; ++j) val[c][j] = (uint32_t)(b + first + j * HS_WAVE);
            continue;
        }
        const uint32_t* src = (const uint32_t*)A.src[1 + c] + b;
#pragma unroll
        for (int j = 0; j < RX_PER; ++j) val[c][j] = first + j * HS_WAVE < rows ? src[first + j * HS_WAVE] : 0u;
    }
    rx_zero<RX_WAVES>(whist, 1 << A.bits);
    __syncthreads();
    const int shift = A.shift, bits = A.bits;
    const uint64_t below = (1ull << lane) - 1ull;
    uint32_t bl[RX_PER];  // bin | rank inside (wave, bin) << 8
#pragma unroll
    for (int j = 0; j < RX_PER; ++j) {
        const bool valid = first + j * HS_WAVE < rows;
        const uint32_t bin = valid ? rx_bin_of(A, key[j], shift, bits) : 0u;
        bl[j] = bin | (rx_rank(whist[w], bin, valid, bits, below) << 8);
    }
    rx_bin_starts(A, T, whist, gbase, s_wave_tot);
    uint32_t at[RX_PER];  // tile-local position of my rows in bin order
#pragma unroll
    for (int j = 0; j < RX_PER; ++j) {
        const bool valid = first + j * HS_WAVE < rows;
        at[j] = valid ? whist[w][bl[j] & 0xffu] + (bl[j] >> 8) : 0xffffffffu;
        if (valid) {
            sbin[at[j]] = (uint8_t)bl[j];
            stage[at[j]] = key[j];
        }
    }
    // this kernel writes its staged columns out in its own words: through rx_write_out the compiler spends 2 more VGPRs
    // (NV = 1) or 4 more bytes of scratch (NV = 2, 3) on it
    __syncthreads();
    {
        int32_t* dst = (int32_t*)A.dst[0];
#pragma unroll
        for (int k = 0; k < RX_PER; ++k) {
            const int i = tid + k * RX_THREADS;
            if (i < rows) dst[gbase[sbin[i]] + i] = (int32_t)stage[i];
        }
    }
#pragma unroll
    for (int c = 0; c < NV; ++c) {
        __syncthreads();  // the previous column has left the stage
#pragma unroll
        for (int j = 0; j < RX_PER; ++j)
            if (at[j] != 0xffffffffu) stage[at[j]] = val[c][j];
        __syncthreads();
        uint32_t* dst = (uint32_t*)A.dst[1 + c];
#pragma unroll
        for (int k = 0; k < RX_PER; ++k) {
            const int i = tid + k * RX_THREADS;
            if (i < rows) dst[gbase[sbin[i]] + i] = stage[i];
        }
    }
}

// ---- the pass for wide STRING keys (round 3) -------------------------------------------------------------------------
// A STRING key of one fixed length 8 .. 16 bytes travels as KW = ceil(length / 4) four-byte word columns (columns 0 .. KW - 1;
// zero-padded; the value columns follow), so its tuples are 4-byte columns like an INTEGER key's and take the same tile
// shape, ranking and 32 KB staging at two workgroups per CU; the bin is cut from a mix of all KW words.  FIRST: the words
// come from the string column itself (any alignment: hs_str_words16), through the row list when there is one.
template <int KW>
struct RxWords {
    uint32_t w[KW];
};
template <bool FIRST, int KW>
__device__ __forceinline__ void rx_words(const RxPass& A, int64_t pos, uint32_t* w) {
    if constexpr (FIRST) {
        const int64_t row = A.sel ? A.sel[pos] : A.row0 + pos;
        uint64_t w0, w1;
        hs_str_words16((const uint8_t*)A.key.data + row * A.key.fixed_len, (uint32_t)A.key.fixed_len, w0, w1);
        w[0] = (uint32_t)w0;
        w[1] = (uint32_t)(w0 >> 32);
        if constexpr (KW > 2) w[2] = (uint32_t)w1;
        if constexpr (KW > 3) w[3] = (uint32_t)(w1 >> 32);
    } else {
#pragma unroll
        for (int k = 0; k < KW; ++k) w[k] = ((const uint32_t*)A.src[k])[pos];
    }
}
template <int KW>
__device__ __forceinline__ uint32_t rx_binw(const uint32_t* w, int shift, int bits) {  // RX_BIN_WORDS
    uint32_t h = rx_mix32(w[0]);
#pragma unroll
    for (int k = 1; k < KW; ++k) h = rx_mix32(h ^ w[k]);
    return (h >> shift) & ((1u << bits) - 1u);
}

template <bool FIRST, int KW>
__global__ void __launch_bounds__(RX_H4_THREADS) k_rx_histw(const RxPass A_kernarg) {
    HS_KERNARG(RxPass, A);
    __shared__ uint32_t hist[RX_H4_THREADS / HS_WAVE][1 << RX_MAX_BITS];
    const int shift = A.shift, bits = A.bits;
    rx_hist_tile<RX_H4_THREADS, 8, RxWords<KW>>(
        A, hist, [&](const RxTile& T, int i, RxWords<KW>& key) { rx_words<FIRST, KW>(A, T.b + i, key.w); },
        [&](const RxWords<KW>& key) { return rx_binw<KW>(key.w, shift, bits); });
}

template <bool FIRST, int KW>
__global__ void __launch_bounds__(RX_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8))) k_rx_scatterw(const RxPass A_kernarg) {
    HS_KERNARG(RxPass, A);
    __shared__ uint32_t whist[RX_WAVES][1 << RX_MAX_BITS];
    __shared__ int64_t gbase[1 << RX_MAX_BITS];
    __shared__ uint32_t s_wave_tot[4];
    __shared__ uint8_t sbin[RX_TILE];
    __shared__ uint32_t stage[RX_TILE];
    RxTile T;
    if (!rx_tile(A, T)) return;
    const int tid = threadIdx.x, lane = tid & (HS_WAVE - 1), w = tid / HS_WAVE;
    const int64_t b = T.b;
    const int rows = T.rows;
    const int first = w * RX_SUB + lane;
    rx_zero<RX_WAVES>(whist, 1 << A.bits);
    const int shift = A.shift, bits = A.bits;
    uint32_t bin8[RX_PER];
    {
        uint32_t words[RX_PER][KW];
#pragma unroll
        for (int j = 0; j < RX_PER; ++j)
            if (first + j * HS_WAVE < rows) rx_words<FIRST, KW>(A, b + first + j * HS_WAVE, words[j]);
#pragma unroll
        for (int j = 0; j < RX_PER; ++j) bin8[j] = first + j * HS_WAVE < rows ? rx_binw<KW>(words[j], shift, bits) : 0u;
    }
    __syncthreads();
    const uint64_t below = (1ull << lane) - 1ull;
    uint32_t bl[RX_PER];  // bin | rank inside (wave, bin) << 8
#pragma unroll
    for (int j = 0; j < RX_PER; ++j) bl[j] = bin8[j] | (rx_rank(whist[w], bin8[j], first + j * HS_WAVE < rows, bits, below) << 8);
    rx_bin_starts(A, T, whist, gbase, s_wave_tot);
    uint32_t at[RX_PER];
#pragma unroll
    for (int j = 0; j < RX_PER; ++j) {
        const bool valid = first + j * HS_WAVE < rows;
        at[j] = valid ? whist[w][bl[j] & 0xffu] + (bl[j] >> 8) : 0xffffffffu;
        if (valid) sbin[at[j]] = (uint8_t)bl[j];
    }
    // one column at a time through the 32 KB stage: key words first (FIRST: cut from the string again - the bytes are in L2),
    // then the value columns
    for (int c = 0; c < A.n_cols; ++c) {
        uint32_t v[RX_PER];
        if (FIRST && c < KW) {
#pragma unroll
            for (int j = 0; j < RX_PER; ++j) {
                uint32_t words[KW] = {};
                if (at[j] != 0xffffffffu) rx_words<FIRST, KW>(A, b + first + j * HS_WAVE, words);
                uint32_t pick = words[0];
#pragma unroll
                for (int k = 1; k < KW; ++k) pick = c == k ? words[k] : pick;
                v[j] = pick;
            }
        } else {
            const uint32_t* src = (const uint32_t*)A.src[c] + b;
#pragma unroll
            for (int j = 0; j < RX_PER; ++j) v[j] = at[j] != 0xffffffffu ? src[first + j * HS_WAVE] : 0u;
        }
        __syncthreads();  // the previous column has left the stage (first column: sbin is complete)
#pragma unroll
        for (int j = 0; j < RX_PER; ++j)
            if (at[j] != 0xffffffffu) stage[at[j]] = v[j];
        rx_write_out((uint32_t*)A.dst[c], stage, sbin, gbase, rows);
    }
}

// the partition pass's output segments: (segment, bin) starts where the first tile's counter of that bin points
__global__ void __launch_bounds__(256) k_rx_next(const int64_t* seg_start, const int64_t* tile_base, int64_t n_seg, int32_t bits,
                                                 const int64_t* scanned, int64_t n, int64_t* out) {
    const int64_t total = n_seg << bits;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx <= total; idx += (int64_t)gridDim.x * blockDim.x) {
        if (idx == total) {
            out[idx] = n;
            continue;
        }
        const int64_t s = idx >> bits, bin = idx & ((1ll << bits) - 1);
        const int64_t nt = tile_base[s + 1] - tile_base[s];
        out[idx] = nt ? scanned[(tile_base[s] << bits) + bin * nt] : seg_start[s];
    }
}

// ---- the fold ---------------------------------------------------------------------------------------------------
struct RxAgg {
    const int64_t* seg_start;  // [n_parts + 1]
    int64_t n_parts;
    const void* src[RX_COLS];      // the partitioned tuples
    int32_t esize[RX_COLS];
    int32_t val_kind[HS_MAX_ACC];  // kind of the carried column behind aggregate a (HS_I32 / F32 / I64 / F64 / U8)
    int32_t carried[HS_MAX_ACC];   // aggregate a -> column 1.. of src, 0: the constant const_cell[a]
    uint64_t const_cell[HS_MAX_ACC];
    hs_agg_spec spec;
    int32_t cap, quantise;
    int32_t debug, last;           // last: no later launch takes what this one cannot hold
    uint64_t* prov_key;            // [n] a partition's groups, from the partition's own start
    uint64_t* prov_key1;           // [n] wide keys: the second word
    void* prov_acc[HS_MAX_ACC];    // [n] each: f32 / i32 when quantising, f64 / i64 bits otherwise
    int64_t* pcount;               // [n_parts] groups of the partition
    uint32_t* flags;
    const int64_t* list;           // second launch: the partitions the small table could not hold ...
    const int64_t* list_count;     // ... and their number (device)
    int64_t* overflow;             // first launch: where such partitions are noted
    int64_t* overflow_count;
};

__device__ __forceinline__ uint64_t rx_widen(uint64_t raw, int kind) {
    switch (kind) {
        case HS_I32: return (uint64_t)(int64_t)(int32_t)(uint32_t)raw;
        case HS_F32: return hs_d2u((double)__uint_as_float((uint32_t)raw));
        default: return raw;  // HS_I64 / HS_F64 cells, HS_U8 zero-extended
    }
}
__device__ __forceinline__ uint64_t rx_raw(const void* src, int esize, int64_t i) {
    return esize == 4 ? (uint64_t)((const uint32_t*)src)[i] : esize == 8 ? ((const uint64_t*)src)[i] : (uint64_t)((const uint8_t*)src)[i];
}

// HIPSPARK_RADIX_STAMPS=1: cycles (s_memtime) a wave spends per phase of k_rx_fold, summed over all waves.  The walk
// marks its phases through its policy: the general fold answers with RxStamps, the SUM fold with RxNoStamps - nothing.
__device__ unsigned long long rx_stamp_acc[8];
enum { RX_T_INIT, RX_T_WAIT, RX_T_SLOT, RX_T_RANK, RX_T_FOLD, RX_T_EMIT, RX_T_PHASES };
struct RxStamps {
    const bool on;
    long long from = 0, t[RX_T_PHASES] = {};
    __device__ __forceinline__ void mark() { from = on ? (long long)clock64() : 0; }  // a phase starts
    __device__ __forceinline__ void lap(int phase) {                                   // ... ends, and the next one starts
        const long long now = on ? (long long)clock64() : 0;
        t[phase] += now - from;
        from = now;
    }
    __device__ __forceinline__ void flush(int lane) const {
        if (!on || lane) return;
        for (int k = 0; k < RX_T_PHASES; ++k) atomicAdd(&rx_stamp_acc[k], (unsigned long long)t[k]);
        atomicAdd(&rx_stamp_acc[RX_T_PHASES], 1ull);
    }
};
struct RxNoStamps {
    __device__ __forceinline__ void mark() {}
    __device__ __forceinline__ void lap(int) {}
    __device__ __forceinline__ void flush(int) const {}
};

constexpr int RX_CHUNK = 4;  // 64-row steps loaded together; the next chunk is in flight while this one is folded

// 8-byte words of LDS one fold wave takes: keys[cap] (a wide key: and keys1[cap], its second word), acc[n_acc][cap] and
// order[cap] (u16).  The plan sizes cap by it, the launch the workgroup's LDS, the kernel carves by it.
__host__ __device__ constexpr size_t rx_fold_words(int cap, int n_acc, bool wide) {
    return (size_t)cap * (1 + (wide ? 1 : 0) + n_acc) + (size_t)cap / 4;
}
struct RxWave {  // a fold wave's tables, and what every step of it needs
    uint64_t* keys;   // [cap]
    uint64_t* keys1;  // [cap] wide keys only
    uint64_t* acc;    // [n_acc][cap]
    uint16_t* order;  // [cap] the slots in the order their keys first appeared = the order the groups are written in
    int cap;
    uint32_t mask;
    uint64_t below;   // the lanes before this one
};

// ONE WAVE per partition, both folds.  The tables are cleared once per wave; after a partition only the slots on its
// order list are reset, so a partition costs its rows and its groups, not the table size.  Rows are taken 64 at a time in
// order, RX_CHUNK steps loaded together; the rows of a step that share a slot (rx_peers) reach the accumulators in lane =
// row order.  The partition's groups go to its own start in first-appearance order.
//
// Up to three launches share a kernel, smallest table first (hs_group_radix_run): a partition that meets more keys than
// 3/4 of a table that is not the last is put on the overflow list instead of being finished; the next launch (A.list set)
// takes the listed partitions; the last table is the one the plan sized for the worst case (every row its own group), and
// outgrowing it raises HS_FLAG_DICT_FULL.
//
// A policy P says what the walk does not know - nothing here depends on the kind of an aggregate:
//   Chunk, load(chunk, base, e, lane)          RX_CHUNK steps of the partition's tuples as registers (0 past the end e)
//   find(T, chunk, j, slot, inserted)          the dictionary slot of step j's row (valid lanes; slot stays -1: no room)
//   fold(T, chunk, j, i, valid, slot, peers)   step j's rows into acc[][slot], every f64 cell in row order
//   n_acc(), is_int(a), identity(a), check(a, cell, err)   the cells: their number, empty value and emit-time check
//   slot_bits(cap), WIDE, stamps
template <typename P>
__device__ __forceinline__ void rx_fold_walk(const RxAgg& A, uint64_t* lds, P pol) {
    const int lane = threadIdx.x & (HS_WAVE - 1), w = threadIdx.x / HS_WAVE, wpb = blockDim.x / HS_WAVE;
    const int NA = pol.n_acc(), cap = A.cap;
    RxWave T;
    T.keys = lds + (size_t)w * rx_fold_words(cap, NA, P::WIDE);
    T.keys1 = T.keys + cap;
    T.acc = T.keys + (P::WIDE ? 2 : 1) * cap;
    T.order = (uint16_t*)(T.acc + (size_t)NA * cap);
    T.cap = cap;
    T.mask = (uint32_t)cap - 1u;
    T.below = (1ull << lane) - 1ull;
    const int limit = A.last ? cap : cap - cap / 4;  // groups a partition may hold in this launch
    const int slot_bits = pol.slot_bits(cap);
    uint32_t err = 0;
    const int64_t n_todo = A.list ? *A.list_count : A.n_parts;
    if ((int64_t)blockIdx.x * wpb + w >= n_todo) return;  // nothing listed for this wave: no table to clear either
    for (int s = lane; s < cap; s += HS_WAVE) T.keys[s] = HS_EMPTY_KEY;
    for (int a = 0; a < NA; ++a) {
        const uint64_t id = pol.identity(a);
        for (int s = lane; s < cap; s += HS_WAVE) T.acc[a * cap + s] = id;
    }
    for (int64_t q = (int64_t)blockIdx.x * wpb + w; q < n_todo; q += (int64_t)gridDim.x * wpb) {
        const int64_t p = A.list ? A.list[q] : q;
        const int64_t b = A.seg_start[p], e = A.seg_start[p + 1];
        if (b >= e) {
            if (lane == 0) A.pcount[p] = 0;
            continue;
        }
        pol.stamps.mark();
        typename P::Chunk next;
        pol.load(next, b, e, lane);
        int ngroups = 0;
        bool full = false;
        pol.stamps.lap(RX_T_INIT);
        for (int64_t base = b; base < e && !full; base += RX_CHUNK * HS_WAVE) {
            pol.stamps.mark();
            const typename P::Chunk cur = next;
            pol.stamps.lap(RX_T_WAIT);  // only the register copy: nothing here waits for the loads, the first use (SLOT) does
            if (base + RX_CHUNK * HS_WAVE < e) pol.load(next, base + RX_CHUNK * HS_WAVE, e, lane);
#pragma unroll
            for (int j = 0; j < RX_CHUNK; ++j) {
                if (base + j * HS_WAVE >= e || full) break;
                const int64_t i = base + j * HS_WAVE + lane;
                const bool valid = i < e;
                pol.stamps.mark();
                int slot = valid ? -1 : 0;
                bool inserted = false;
                if (valid) pol.find(T, cur, j, slot, inserted);
                const uint64_t fresh = __ballot(inserted);
                if (inserted) T.order[ngroups + __popcll(fresh & T.below)] = (uint16_t)slot;
                ngroups += __popcll(fresh);
                if (ngroups > limit || __ballot(valid && slot < 0) != 0ull) {  // too many keys for this table
                    full = true;
                    break;
                }
                pol.stamps.lap(RX_T_SLOT);
                const uint64_t peers = rx_peers((uint32_t)slot, valid, slot_bits);
                pol.stamps.lap(RX_T_RANK);
                pol.fold(T, cur, j, i, valid, slot, peers);
                pol.stamps.lap(RX_T_FOLD);
            }
        }
        pol.stamps.mark();
        if (full) {
            // leave the partition to the launch with the next table (or, from the last one, to the caller's other path)
            if (A.last) err |= HS_FLAG_DICT_FULL;
            else if (lane == 0) A.overflow[atomicAdd((unsigned long long*)A.overflow_count, 1ull)] = p;
            if (lane == 0) A.pcount[p] = 0;
        }
        // the partition's groups, in the order their keys first appeared, from the partition's own start; their slots reset
        for (int g0 = 0; g0 < ngroups; g0 += HS_WAVE) {
            const int g = g0 + lane;
            if (g >= ngroups) continue;
            const int s = T.order[g];
            const int64_t at = b + g;
            if (!full) A.prov_key[at] = T.keys[s];
            if (P::WIDE && !full) A.prov_key1[at] = T.keys1[s];
            T.keys[s] = HS_EMPTY_KEY;
            for (int a = 0; a < NA; ++a) {
                const bool is_int = pol.is_int(a);
                uint64_t v = T.acc[a * cap + s];
                T.acc[a * cap + s] = pol.identity(a);
                if (full) continue;
                pol.check(a, v, err);
                if (A.quantise) {
                    v = hs_quantise_cell(is_int, v, err);
                    if (is_int) ((int32_t*)A.prov_acc[a])[at] = (int32_t)(int64_t)v;
                    else ((float*)A.prov_acc[a])[at] = (float)hs_u2d(v);
                } else {
                    ((uint64_t*)A.prov_acc[a])[at] = v;
                }
            }
        }
        if (!full && lane == 0) A.pcount[p] = ngroups;
        pol.stamps.lap(RX_T_EMIT);
    }
    if (err) atomicOr(A.flags, err);
    pol.stamps.flush(lane);
}

// ---- the general fold: any operator over any cell kind ------------------------------------------------------------------
// NC = value columns that travel with the rows (0 .. 4 specialised: the tuples of a chunk sit in registers; -1: any
// number, one global round trip per step and column).  SLOT_BITS >= log2(cap): 9 for the small tables, 12 for the large.
// A group's first lane of a step folds the values of all its lanes, in lane order, collecting them by shuffle.
template <int NC, int SLOT_BITS>
struct RxFoldAny {
    static constexpr bool WIDE = false;
    struct Chunk {
        uint64_t k[RX_CHUNK], x[RX_CHUNK][NC > 0 ? NC : 1];
    };
    const RxAgg& A;
    RxStamps stamps;
    __device__ __forceinline__ int n_acc() const { return A.spec.n_acc; }
    __device__ __forceinline__ int slot_bits(int) const { return SLOT_BITS; }
    __device__ __forceinline__ bool is_int(int a) const { return A.spec.is_int[a] != 0; }
    __device__ __forceinline__ uint64_t identity(int a) const { return hs_acc_identity(A.spec.op[a], is_int(a)); }
    __device__ __forceinline__ void check(int a, uint64_t cell, uint32_t& err) const {
        if (hs_float_identity_left(A.spec.op[a], is_int(a), cell)) err |= HS_FLAG_TYPE_ASSERT;
    }
    __device__ __forceinline__ void load(Chunk& n, int64_t base, int64_t e, int lane) const {
#pragma unroll
        for (int j = 0; j < RX_CHUNK; ++j) {
            const int64_t i = base + j * HS_WAVE + lane;
            const bool valid = i < e;
            n.k[j] = !valid ? 0 : (A.esize[0] == 4 ? (uint64_t)(int64_t)((const int32_t*)A.src[0])[i] : ((const uint64_t*)A.src[0])[i]);
            n.x[j][0] = 0;
#pragma unroll
            for (int c = 0; c < NC; ++c) n.x[j][c] = valid ? rx_raw(A.src[1 + c], A.esize[1 + c], i) : 0;
        }
    }
    __device__ __forceinline__ void find(const RxWave& T, const Chunk& ch, int j, int& slot, bool& inserted) const {
        const uint64_t k = ch.k[j];
        uint32_t h = (uint32_t)(hs_mix64(k) >> 36) & T.mask;
        for (uint32_t probe = 0; probe <= T.mask; ++probe) {
            uint64_t cur = __hip_atomic_load(&T.keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (cur == HS_EMPTY_KEY) {
                cur = atomicCAS((unsigned long long*)&T.keys[h], (unsigned long long)HS_EMPTY_KEY, (unsigned long long)k);
                if (cur == HS_EMPTY_KEY) {
                    cur = k;
                    inserted = true;
                }
            }
            if (cur == k) {
                slot = (int)h;
                break;
            }
            h = (h + 1) & T.mask;
        }
    }
    __device__ __forceinline__ void fold(const RxWave& T, const Chunk& ch, int j, int64_t i, bool valid, int slot, uint64_t peers) const {
        const int lane = threadIdx.x & (HS_WAVE - 1), NA = A.spec.n_acc;
        const bool leader = valid && (peers & T.below) == 0ull;
        const uint64_t crowded = __ballot(valid && __popcll(peers) > 1);
        for (int a = 0; a < NA; ++a) {
            const uint32_t op = A.spec.op[a];
            const bool is_int = A.spec.is_int[a] != 0;
            const int c = A.carried[a];
            uint64_t x = A.const_cell[a];
            if (c) {
                uint64_t raw = 0;
                if constexpr (NC > 0) {
#pragma unroll
                    for (int cc = 0; cc < NC; ++cc)
                        if (c - 1 == cc) raw = ch.x[j][cc];
                } else {
                    raw = valid ? rx_raw(A.src[c], A.esize[c], i) : 0;
                }
                x = rx_widen(raw, A.val_kind[a]);
            }
            uint64_t v = 0;
            if (leader) v = hs_acc_fold(op, is_int, T.acc[a * T.cap + slot], x);
            if (crowded) {
                uint64_t rest = leader ? peers & ~(1ull << lane) : 0ull;
                while (__ballot(rest != 0ull) != 0ull) {
                    const int from = rest ? __ffsll((long long)rest) - 1 : lane;
                    const uint64_t xv = __shfl(x, from, HS_WAVE);
                    if (rest) {
                        v = hs_acc_fold(op, is_int, v, xv);
                        rest &= rest - 1;
                    }
                }
            }
            if (leader) T.acc[a * T.cap + slot] = v;
        }
    }
};
template <int NC, int SLOT_BITS>
__global__ void __launch_bounds__(256) k_rx_fold(const RxAgg A_kernarg) {
    HS_KERNARG(RxAgg, A);
    extern __shared__ __align__(16) uint64_t rx_lds[];
    rx_fold_walk(A, rx_lds, RxFoldAny<NC, SLOT_BITS>{A, {A.debug != 0}});
}

// ---- the fold, specialised for SUMs (round 3) ---------------------------------------------------------------------
// What SUM / AVG / COUNT lower to: every aggregate is a SUM whose argument is an f32 column (class 0: f64 cell), an i32
// column (class 1: i64 cell) or an integer constant (class 2: COUNT).  The same walk and the same order of additions as
// the general fold - a group's f64 cell takes its rows' values in row order - at about a quarter of the instructions: the
// classes are compile-time (no per-value switches on kind and operator), the dictionary probe is the compare-and-swap
// itself, values travel as the 32 bits they are, and the rows of a step that share a group are folded in RANK ROUNDS -
// round r: the lanes whose rank among their group's lanes is r add their value to the group's cell in LDS (distinct cells
// within a round; LDS executes a wave's instructions in order, so round r + 1 reads what round r wrote) - instead of a
// leader lane collecting its peers' values with shuffles.  Integer cells are order-free: one LDS atomic per lane (COUNT:
// one per group and step, with the group's lane count).
// CLS: two bits of class per aggregate.  KM: 0 = 4-byte key column, 1 = 8-byte key words, 2 .. 4 = a wide STRING key in
// that many 4-byte word columns (compared as two 64-bit words; the value columns follow the key's)
constexpr int rx_sum_class(int cls, int a) { return (cls >> (2 * a)) & 3; }
constexpr int rx_sum_col(int cls, int a) {  // carried columns are numbered in aggregate order (hs_group_radix_run)
    int c = 0;
    for (int k = 0; k < a; ++k) c += rx_sum_class(cls, k) < 2 ? 1 : 0;
    return c;
}
template <int NA, int CLS, int KM>
struct RxFoldSum {
    static constexpr bool WIDE = KM >= 2, KEY4 = KM == 0 || WIDE;
    static constexpr int KW = WIDE ? KM : 1, NC = rx_sum_col(CLS, NA);
    using KeyReg = std::conditional_t<KEY4, uint32_t, uint64_t>;  // as loaded: widening a key right after its load would wait for it
    struct Chunk {
        KeyReg k[RX_CHUNK];
        uint32_t w[RX_CHUNK][KW];  // WIDE: key words 1 .. KW - 1 ([0] unused)
        uint32_t x[RX_CHUNK][NC > 0 ? NC : 1];
    };
    const RxAgg& A;
    RxNoStamps stamps;
    __device__ __forceinline__ int n_acc() const { return NA; }
    __device__ __forceinline__ int slot_bits(int cap) const {
        int bits = 0;
        while ((1 << bits) < cap) ++bits;
        return bits;
    }
    __device__ __forceinline__ bool is_int(int a) const { return rx_sum_class(CLS, a) != 0; }
    __device__ __forceinline__ uint64_t identity(int) const { return 0; }  // of SUM, f64 and i64 alike
    __device__ __forceinline__ void check(int, uint64_t, uint32_t&) const {}
    __device__ __forceinline__ void load(Chunk& n, int64_t base, int64_t e, int lane) const {
#pragma unroll
        for (int j = 0; j < RX_CHUNK; ++j) {
            const int64_t i = base + j * HS_WAVE + lane;
            const bool valid = i < e;
            n.k[j] = valid ? ((const KeyReg*)A.src[0])[i] : 0;
            n.w[j][0] = n.x[j][0] = 0u;
#pragma unroll
            for (int q = 1; q < KW; ++q) n.w[j][q] = valid ? ((const uint32_t*)A.src[q])[i] : 0u;
#pragma unroll
            for (int c = 0; c < NC; ++c) n.x[j][c] = valid ? ((const uint32_t*)A.src[KW + c])[i] : 0u;
        }
    }
    __device__ __forceinline__ void find(const RxWave& T, const Chunk& ch, int j, int& slot, bool& inserted) const {
        uint64_t k, k1 = 0;
        if constexpr (WIDE) {
            k = (uint64_t)ch.k[j] | ((uint64_t)ch.w[j][1] << 32);
            if constexpr (KW > 2) k1 = (uint64_t)ch.w[j][2];
            if constexpr (KW > 3) k1 |= (uint64_t)ch.w[j][3] << 32;
        } else {
            k = KEY4 ? (uint64_t)(int64_t)(int32_t)ch.k[j] : (uint64_t)ch.k[j];
        }
        uint32_t h;
        if constexpr (KEY4 && !WIDE) {  // two 32-bit multiplies; bits independent of the ones the partitions were cut on
            uint32_t m = (uint32_t)k * 0xCC9E2D51u;
            m ^= m >> 17;
            h = ((m * 0x1B873593u) >> 12) & T.mask;
        } else if constexpr (WIDE) {
            h = (uint32_t)(hs_mix64(k ^ hs_mix64(k1)) >> 36) & T.mask;
        } else {
            h = (uint32_t)(hs_mix64(k) >> 36) & T.mask;
        }
        // no break: the loop ends on slot >= 0, so its body stays one block of selects (with a break in it the compiler
        // keeps a branch per probe round, which costs the many-keys shapes 3-4 % of the tier)
        for (uint32_t probe = 0; probe <= T.mask && slot < 0; ++probe) {
            const uint64_t cur = atomicCAS((unsigned long long*)&T.keys[h], (unsigned long long)HS_EMPTY_KEY, (unsigned long long)k);
            bool mine = cur == HS_EMPTY_KEY || cur == k;
            if constexpr (WIDE) {
                // the lane that claimed the slot completes it before any lane of the wave - this probe round or a
                // later one - compares the second word (LDS executes the wave's instructions in order)
                if (cur == HS_EMPTY_KEY) T.keys1[h] = k1;
                rx_wave_handover();
                mine = cur == HS_EMPTY_KEY || (cur == k && T.keys1[h] == k1);
            }
            inserted = mine && cur == HS_EMPTY_KEY;
            slot = mine ? (int)h : -1;
            h = (h + 1) & T.mask;
        }
    }
    __device__ __forceinline__ void fold(const RxWave& T, const Chunk& ch, int j, int64_t, bool valid, int slot, uint64_t peers) const {
        constexpr bool any_float = (NA > 0 && rx_sum_class(CLS, 0) == 0) || (NA > 1 && rx_sum_class(CLS, 1) == 0) ||
                                   (NA > 2 && rx_sum_class(CLS, 2) == 0);
        const int rank = valid ? __popcll(peers & T.below) : -1;
        // the group's cell of aggregate a is mine[a * cap]: ONE per-lane address and uniform offsets (written as
        // acc[a * cap + slot] the compiler keeps a per-lane base per aggregate alive through the whole walk: +4 VGPRs)
        uint64_t* mine = T.acc + slot;
#pragma unroll
        for (int a = 0; a < NA; ++a) {  // integer cells: any order
            if (rx_sum_class(CLS, a) == 1) {
                if (valid) atomicAdd((unsigned long long*)&mine[a * T.cap], (unsigned long long)(int64_t)(int32_t)ch.x[j][rx_sum_col(CLS, a)]);
            } else if (rx_sum_class(CLS, a) == 2) {
                if (rank == 0) atomicAdd((unsigned long long*)&mine[a * T.cap], A.const_cell[a] * (uint64_t)__popcll(peers));
            }
        }
        if constexpr (any_float) {
            for (int r = 0; __ballot(rank == r) != 0ull; ++r) {
                if (rank == r) {
#pragma unroll
                    for (int a = 0; a < NA; ++a) {
                        if (rx_sum_class(CLS, a) != 0) continue;
                        uint64_t* cell = &mine[a * T.cap];
                        *cell = hs_d2u(hs_u2d(*cell) + (double)__uint_as_float(ch.x[j][rx_sum_col(CLS, a)]));
                    }
                }
                rx_wave_handover();
            }
        }
    }
};
template <int NA, int CLS, int KM>
__global__ void __launch_bounds__(256) k_rx_fold_sum(const RxAgg A_kernarg) {
    HS_KERNARG(RxAgg, A);
    extern __shared__ __align__(16) uint64_t rx_lds[];
    rx_fold_walk(A, rx_lds, RxFoldSum<NA, CLS, KM>{A, {}});
}

// ---- dense output -----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_rx_unit_groups(const int64_t* pscan, int64_t parts_per_unit, int32_t n_units,
                                                        int64_t* out) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u <= n_units) out[u] = pscan[(int64_t)u * parts_per_unit];
}

struct RxEmit {
    const int64_t* seg_start;
    const int64_t* pscan;
    int64_t n_parts;
    const uint64_t* prov_key;
    const uint64_t* prov_key1;
    const void* prov_acc[HS_MAX_ACC];
    int32_t n_acc, osize, key_kind, pad;
    void* out_key;
    void* out_acc[HS_MAX_ACC];
};
__global__ void __launch_bounds__(256) k_rx_emit(const RxEmit A_kernarg) {
    HS_KERNARG(RxEmit, A);
    const int lane = threadIdx.x & (HS_WAVE - 1), wpb = blockDim.x / HS_WAVE;
    for (int64_t p = (int64_t)blockIdx.x * wpb + threadIdx.x / HS_WAVE; p < A.n_parts; p += (int64_t)gridDim.x * wpb) {
        const int64_t from = A.seg_start[p], to = A.pscan[p], cnt = A.pscan[p + 1] - to;
        for (int64_t q = lane; q < cnt; q += HS_WAVE) {
            const uint64_t k = A.prov_key[from + q];
            const int base = A.key_kind & 0xff;
            if (base == HS_I32) ((int32_t*)A.out_key)[to + q] = (int32_t)(int64_t)k;
            else if (base == HS_F32) ((float*)A.out_key)[to + q] = (float)hs_u2d(k);  // the word: the f32 widened, exactly
            else if (base == HS_STR) {
                const int len = A.key_kind >> 8;  // hs_pack_str / hs_str_words16: byte i of the string = byte i of the word(s)
                const uint64_t k1 = len > 8 ? A.prov_key1[from + q] : 0ull;
                for (int i = 0; i < len; ++i)
                    ((uint8_t*)A.out_key)[(to + q) * len + i] = (uint8_t)(i < 8 ? k >> (8 * i) : k1 >> (8 * (i - 8)));
            } else ((uint64_t*)A.out_key)[to + q] = k;
            for (int a = 0; a < A.n_acc; ++a) rx_move(A.prov_acc[a], A.out_acc[a], A.osize, from + q, to + q);
        }
    }
}

// ---- host -------------------------------------------------------------------------------------------------------
static int rx_esize(int32_t kind) {
    switch (kind) {
        case HS_I32:
        case HS_F32: return 4;
        case HS_I64:
        case HS_F64: return 8;
        case HS_U8: return 1;
        default: return 0;
    }
}
static size_t rx_align(size_t x) { return (x + 255) & ~(size_t)255; }

// key_kind of a plan: a STRING key of one fixed length 8 .. 16 bytes = two key words per tuple
static int rx_plan_wide(int64_t key_kind) {  // -> number of 4-byte key word columns (2 .. 4), 0: not a wide key
    return (key_kind & 0xff) == HS_STR && (key_kind >> 8) > 7 ? (int)(((key_kind >> 8) + 3) / 4) : 0;
}

// field use of the public plan (include/hipspark.h keeps it opaque: int64 f[48])
enum {
    PL_N, PL_UNITS, PL_BITS1, PL_BITS2, PL_CAP, PL_NA, PL_NCARRIED, PL_QUANTISE, PL_KEYKIND, PL_NSEG1, PL_PARTS, PL_TILES1,
    PL_TILES2, PL_COUNTERS, PL_OSIZE, PL_WS, PL_OFF_BUF_A, PL_OFF_BUF_B, PL_OFF_SEG1, PL_OFF_SEG2, PL_OFF_TB0, PL_OFF_TB1,
    PL_OFF_CNT, PL_OFF_SCAN, PL_OFF_SCANWS, PL_OFF_PKEY, PL_OFF_PACC, PL_OFF_PCOUNT, PL_OFF_PSCAN, PL_OFF_OVERFLOW, PL_TUPLE, PL_ESIZE0 /* .. +16 */
};

// the instantiations of the pass's specialised kernels, by [KW - 2][FIRST], [NV][FIRST] and [FIRST]
using RxKernel = void (*)(const RxPass);
static constexpr RxKernel RX_HISTW[3][2] = {{k_rx_histw<false, 2>, k_rx_histw<true, 2>},
                                            {k_rx_histw<false, 3>, k_rx_histw<true, 3>},
                                            {k_rx_histw<false, 4>, k_rx_histw<true, 4>}};
static constexpr RxKernel RX_SCATTERW[3][2] = {{k_rx_scatterw<false, 2>, k_rx_scatterw<true, 2>},
                                               {k_rx_scatterw<false, 3>, k_rx_scatterw<true, 3>},
                                               {k_rx_scatterw<false, 4>, k_rx_scatterw<true, 4>}};
static constexpr RxKernel RX_HIST4[2] = {k_rx_hist4<false>, k_rx_hist4<true>};
static constexpr RxKernel RX_SCATTER4[4][2] = {{k_rx_scatter4<0, false>, k_rx_scatter4<0, true>},
                                               {k_rx_scatter4<1, false>, k_rx_scatter4<1, true>},
                                               {k_rx_scatter4<2, false>, k_rx_scatter4<2, true>},
                                               {k_rx_scatter4<3, false>, k_rx_scatter4<3, true>}};
// ... and of the folds.  The general one by [carried columns 0 .. 4, 5: any number][cap <= 512 ? 0 : 1]:
using RxFoldKernel = void (*)(const RxAgg);
static constexpr RxFoldKernel RX_FOLD[6][2] = {{k_rx_fold<0, 9>, k_rx_fold<0, 12>}, {k_rx_fold<1, 9>, k_rx_fold<1, 12>},
                                               {k_rx_fold<2, 9>, k_rx_fold<2, 12>}, {k_rx_fold<3, 9>, k_rx_fold<3, 12>},
                                               {k_rx_fold<4, 9>, k_rx_fold<4, 12>}, {k_rx_fold<-1, 9>, k_rx_fold<-1, 12>}};
// the SUM fold by [n_acc - 1][class code: two bits per aggregate, 0 .. 2 each][key mode 0 .. 4]: 3 + 9 + 27 class codes
// x 5 key modes are kernels, every other cell (a class 3, a class beyond n_acc) is null
constexpr int RX_SUM_CODES = 64, RX_SUM_KM = 5;
constexpr bool rx_sum_code_ok(int n_acc, int code) {
    for (int a = 0; a < 3; ++a)
        if (a < n_acc ? rx_sum_class(code, a) > 2 : rx_sum_class(code, a) != 0) return false;
    return true;
}
template <int NA, int CLS, int KM>
constexpr RxFoldKernel rx_sum_kernel() {
    if constexpr (rx_sum_code_ok(NA, CLS)) return k_rx_fold_sum<NA, CLS, KM>;
    else return nullptr;
}
struct RxSumTable {
    RxFoldKernel k[3][RX_SUM_CODES][RX_SUM_KM];
};
template <size_t... I>
constexpr RxSumTable rx_sum_table(std::index_sequence<I...>) {
    RxSumTable t{};
    ((t.k[I / (RX_SUM_CODES * RX_SUM_KM)][I / RX_SUM_KM % RX_SUM_CODES][I % RX_SUM_KM] =
          rx_sum_kernel<(int)(I / (RX_SUM_CODES * RX_SUM_KM)) + 1, (int)(I / RX_SUM_KM % RX_SUM_CODES), (int)(I % RX_SUM_KM)>()),
     ...);
    return t;
}
static constexpr RxSumTable RX_FOLD_SUM = rx_sum_table(std::make_index_sequence<3 * RX_SUM_CODES * RX_SUM_KM>{});

// one partition pass over the segments of `pass`: tiles, histogram, scan, scatter, the next level's segments
static int rx_pass(hipStream_t stream, const RxPass& pass, int64_t max_tiles, int64_t* counters, int64_t* scanned, void* scan_ws,
                   int64_t n, int64_t* next_seg) {
    RxPass P = pass;
    hipLaunchKernelGGL(k_rx_tiles, dim3(1), dim3(1024), 0, stream, P.seg_start, P.n_seg, (int64_t*)P.tile_base);
    RX_CHECK_LAUNCH("radix pass (tiles)");
    const int64_t ncnt = max_tiles << P.bits;
    hs_memset_async(counters, 0, (size_t)ncnt * 8, stream);
    P.counters = counters;
    // which kernels: a wide key's; for 4-byte tuples (INTEGER key, f32 / i32 values; not the raw sorts, whose bins are
    // cut from 64-bit words) the specialised ones, and a key mix becomes the 32-bit one; else the generic pair
    const int first = P.first ? 1 : 0, wide = P.mode == RX_BIN_WORDS ? P.wide : 0;
    bool four = !wide && P.mode != RX_BIN_PLUS1 && P.mode != RX_BIN_VALUE && P.n_cols <= 4 &&
                (first ? P.key.kind == HS_I32 : P.esize[0] == 4);
    for (int c = 1; c < P.n_cols; ++c) four = four && P.esize[c] == 4;
    if (four && P.mode == RX_BIN_MIX64) P.mode = RX_BIN_MIX32;
    int widest = 1;
    for (int c = 0; c < P.n_cols; ++c) widest = P.esize[c] > widest ? P.esize[c] : widest;
    auto launch = [&](const char* what, RxKernel kernel, int threads, size_t dynamic_lds) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)max_tiles), dim3(threads), dynamic_lds, stream, P);
        if (hipGetLastError() == hipSuccess) return HS_OK;
        hs_set_error("radix pass (%s): kernel launch failed", what);
        return HS_E_LAUNCH;
    };
    int rc = launch("histogram", wide ? RX_HISTW[wide - 2][first] : four ? RX_HIST4[first] : k_rx_hist, wide || four ? RX_H4_THREADS : RX_THREADS, 0);
    if (rc != HS_OK) return rc;
    rc = hs_exclusive_scan_i64(stream, counters, ncnt, scanned, scan_ws);
    if (rc != HS_OK) return rc;
    P.counters = scanned;
    static unsigned long long attr_set = 0;
    if (hs_first_on_device(attr_set))  // 8-byte columns stage 72 KB + 18 KB static: above the 64 KB a launch gets unasked
        (void)hipFuncSetAttribute((const void*)k_rx_scatter, hipFuncAttributeMaxDynamicSharedMemorySize, RX_TILE * 9);
    rc = launch("scatter", wide ? RX_SCATTERW[wide - 2][first] : four ? RX_SCATTER4[P.n_cols - 1][first] : k_rx_scatter, RX_THREADS,
                wide || four ? 0 : (size_t)RX_TILE * (1 + widest));
    if (rc != HS_OK) return rc;
    if (next_seg) {
        const int64_t nout = (P.n_seg << P.bits) + 1;
        hipLaunchKernelGGL(k_rx_next, dim3((unsigned)((nout + 255) / 256 > 4096 ? 4096 : (nout + 255) / 256)), dim3(256), 0, stream,
                           P.seg_start, P.tile_base, P.n_seg, (int32_t)P.bits, (const int64_t*)scanned, n, next_seg);
        RX_CHECK_LAUNCH("radix pass (segments)");
    }
    return HS_OK;
}

extern "C" int hs_group_radix_plan(int32_t key_kind, int64_t n, int32_t n_units, int64_t max_unit_rows, const int32_t* val_kinds,
                                   const hs_agg_spec* spec, int32_t quantise, hs_radix_plan* plan) {
    if (!plan || !spec || n < 1 || n_units < 1 || max_unit_rows < 1 || spec->n_acc < 0 || spec->n_acc > HS_MAX_ACC ||
        (spec->n_acc > 0 && !val_kinds)) {
        hs_set_error("hs_group_radix_plan: bad arguments");
        return HS_E_ARG;
    }
    {   // keys whose 64-bit key word IS the key: integers, floats (0.0 == -0.0, as one Python dict key), strings of a fixed
        // length <= 7 bytes (key_kind = HS_STR + 256 x length)
        const int base = key_kind & 0xff, len = key_kind >> 8;
        const bool ok = base == HS_STR ? (len >= 1 && len <= 16) : (len == 0 && (base == HS_I32 || base == HS_I64 || base == HS_F32 || base == HS_F64));
        if (!ok) {
            hs_set_error("hs_group_radix_plan: key kind %d (HS_I32 / I64 / F32 / F64, or HS_STR + 256 x fixed length <= 16)", (int)key_kind);
            return HS_E_LIMIT;
        }
    }
    // strings of 8 .. 16 bytes travel as 2 .. 4 four-byte key word columns and are compared on all of them: exact, no
    // hashing.  Only the SUM-specialised fold knows them: SUM / AVG / COUNT over f32 / i32 columns and integer constants,
    // <= 3 aggregates
    const int wide = rx_plan_wide(key_kind);
    if (wide) {
        bool sums = spec->n_acc >= 1 && spec->n_acc <= 3;
        for (int a = 0; a < spec->n_acc && sums; ++a) {
            const bool is_int = spec->is_int[a] != 0;
            sums = spec->op[a] == HS_AGG_SUM && ((val_kinds[a] == HS_F32 && !is_int) || (val_kinds[a] == HS_I32 && is_int) || (val_kinds[a] < 0 && is_int));
        }
        if (!sums) {
            hs_set_error("hs_group_radix_plan: a STRING key of 8 .. 16 bytes needs SUM / COUNT aggregates over f32 / i32 columns (<= 3)");
            return HS_E_LIMIT;
        }
    }
    int64_t* f = plan->f;
    for (int i = 0; i < 48; ++i) f[i] = 0;
    const int NA = spec->n_acc;
    int cap = 2048;
    while (cap > 64 && rx_fold_words(cap, NA, wide != 0) * 8 > 65536) cap >>= 1;
    // rows per partition: half the slots of the LARGE table.  Partitions that turn out to hold few distinct keys - the
    // usual case - are folded by the 512-slot launch anyway.  (Cutting down to half the slots of the SMALL table where two
    // passes can was measured at 600 M rows / 287 units: all-distinct keys 2.2x faster - no partition needs the large-table
    // launch -, but ~100 rows per group 65 % slower - a finer cut puts more rows of a group into every 64-row step, and
    // those fold one after the other - and 4 rows per group 10 % slower: not taken.)
    int bits = 0;
    while (bits < 2 * RX_MAX_BITS && ((int64_t)(cap / 2) << bits) < max_unit_rows) ++bits;
    const int bits1 = bits <= RX_MAX_BITS ? bits : (bits + 1) / 2, bits2 = bits - bits1;
    f[PL_N] = n;
    f[PL_UNITS] = n_units;
    f[PL_BITS1] = bits1;
    f[PL_BITS2] = bits2;
    f[PL_CAP] = cap;
    f[PL_NA] = NA;
    f[PL_QUANTISE] = quantise ? 1 : 0;
    f[PL_KEYKIND] = key_kind;
    f[PL_NSEG1] = (int64_t)n_units << bits1;
    f[PL_PARTS] = (int64_t)n_units << bits;
    f[PL_TILES1] = n / RX_TILE + n_units + 1;
    f[PL_TILES2] = bits2 ? n / RX_TILE + f[PL_NSEG1] + 1 : 0;
    const int64_t c1 = f[PL_TILES1] << bits1, c2 = f[PL_TILES2] << bits2;
    f[PL_COUNTERS] = c1 > c2 ? c1 : c2;
    f[PL_OSIZE] = quantise ? 4 : 8;
    f[PL_ESIZE0] = key_kind == HS_I32 || wide ? 4 : 8;
    const int kcols = wide ? wide : 1;  // key columns of a tuple; the value columns follow
    for (int q = 1; q < kcols; ++q) f[PL_ESIZE0 + q] = 4;
    int64_t tuple = f[PL_ESIZE0] * kcols;
    int carried = 0;
    for (int a = 0; a < NA; ++a) {
        if (val_kinds[a] < 0) continue;  // a constant: does not travel
        const int es = rx_esize(val_kinds[a]);
        if (!es) {
            hs_set_error("hs_group_radix_plan: value column %d has kind %d", a, (int)val_kinds[a]);
            return HS_E_ARG;
        }
        f[PL_ESIZE0 + kcols + carried] = es;
        tuple += es;
        ++carried;
    }
    f[PL_NCARRIED] = carried;
    f[PL_TUPLE] = tuple;
    size_t off = 0;
    auto take = [&](int field, size_t bytes) {
        f[field] = (int64_t)off;
        off += rx_align(bytes);
    };
    // a buffer set = the columns back to back, each n elements
    size_t set_bytes = 0;
    for (int c = 0; c < kcols + carried; ++c) set_bytes += rx_align((size_t)n * f[PL_ESIZE0 + c]);
    take(PL_OFF_BUF_A, set_bytes);
    take(PL_OFF_BUF_B, bits2 ? set_bytes : 0);
    take(PL_OFF_SEG1, (size_t)(f[PL_NSEG1] + 1) * 8);
    take(PL_OFF_SEG2, bits2 ? (size_t)(f[PL_PARTS] + 1) * 8 : 0);
    take(PL_OFF_TB0, (size_t)(n_units + 1) * 8);
    take(PL_OFF_TB1, bits2 ? (size_t)(f[PL_NSEG1] + 1) * 8 : 0);
    take(PL_OFF_CNT, (size_t)f[PL_COUNTERS] * 8);
    take(PL_OFF_SCAN, (size_t)(f[PL_COUNTERS] + 1) * 8);
    const int64_t scan_n = f[PL_COUNTERS] > f[PL_PARTS] ? f[PL_COUNTERS] : f[PL_PARTS];
    take(PL_OFF_SCANWS, hs_scan_ws_bytes(scan_n));
    take(PL_OFF_PKEY, (size_t)n * 8 * (wide ? 2 : 1));
    take(PL_OFF_PACC, (size_t)NA * rx_align((size_t)n * f[PL_OSIZE]));
    take(PL_OFF_PCOUNT, (size_t)f[PL_PARTS] * 8);
    take(PL_OFF_PSCAN, (size_t)(f[PL_PARTS] + 1) * 8);
    take(PL_OFF_OVERFLOW, (size_t)(f[PL_PARTS] + 1) * 16);  // two lists: past the 256-slot tables, past the 512-slot tables
    f[PL_WS] = (int64_t)off;
    return HS_OK;
}

extern "C" size_t hs_group_radix_ws_bytes(const hs_radix_plan* plan) { return plan ? (size_t)plan->f[PL_WS] : 0; }

static void rx_set_cols(const int64_t* f, uint8_t* ws, int field, void** cols) {
    size_t off = (size_t)f[field];
    for (int c = 0; c < (rx_plan_wide(f[PL_KEYKIND]) ? rx_plan_wide(f[PL_KEYKIND]) : 1) + (int)f[PL_NCARRIED]; ++c) {
        cols[c] = ws + off;
        off += rx_align((size_t)f[PL_N] * f[PL_ESIZE0 + c]);
    }
}

extern "C" int hs_group_radix_run(void* stream_, const hs_radix_plan* plan, const hs_col* key, const int64_t* sel, int64_t row0,
                                  const int64_t* unit_bounds, const hs_col* val_cols, const uint64_t* const_cells,
                                  const hs_agg_spec* spec, void* ws_, int64_t* out_unit_groups, uint32_t* flags) {
    if (!plan || !key || !unit_bounds || !spec || !ws_ || !out_unit_groups || !flags || spec->n_acc != (int)plan->f[PL_NA] ||
        key->kind != (int32_t)(plan->f[PL_KEYKIND] & 0xff) || (key->kind == HS_STR && key->fixed_len != (int32_t)(plan->f[PL_KEYKIND] >> 8)) ||
        (spec->n_acc > 0 && (!val_cols || !const_cells))) {
        hs_set_error("hs_group_radix_run: bad arguments");
        return HS_E_ARG;
    }
    if (hs_refuse_narrow("hs_group_radix_run", key, 1) || hs_refuse_narrow("hs_group_radix_run", val_cols, spec->n_acc)) return HS_E_ARG;
    const int64_t* f = plan->f;
    hipStream_t stream = (hipStream_t)stream_;
    uint8_t* ws = (uint8_t*)ws_;
    const int NA = (int)f[PL_NA], bits1 = (int)f[PL_BITS1], bits2 = (int)f[PL_BITS2], n_units = (int)f[PL_UNITS];
    const int64_t n = f[PL_N];
    void* buf_a[RX_COLS];
    void* buf_b[RX_COLS];
    rx_set_cols(f, ws, PL_OFF_BUF_A, buf_a);
    if (bits2) rx_set_cols(f, ws, PL_OFF_BUF_B, buf_b);
    int64_t* seg1 = (int64_t*)(ws + f[PL_OFF_SEG1]);
    int64_t* seg2 = bits2 ? (int64_t*)(ws + f[PL_OFF_SEG2]) : seg1;
    int64_t* tb0 = (int64_t*)(ws + f[PL_OFF_TB0]);
    int64_t* tb1 = (int64_t*)(ws + f[PL_OFF_TB1]);
    int64_t* counters = (int64_t*)(ws + f[PL_OFF_CNT]);
    int64_t* scanned = (int64_t*)(ws + f[PL_OFF_SCAN]);
    void* scan_ws = ws + f[PL_OFF_SCANWS];

    RxAgg G;
    std::memset(&G, 0, sizeof(G));
    RxPass P;
    std::memset(&P, 0, sizeof(P));
    const int wide = rx_plan_wide(f[PL_KEYKIND]);
    const int kcols = wide ? wide : 1;
    P.n_cols = kcols + (int)f[PL_NCARRIED];
    P.wide = wide;
    P.mode = wide ? RX_BIN_WORDS : RX_BIN_MIX64;
    P.key = *key;
    P.sel = sel;
    P.row0 = row0;
    for (int c = 0; c < P.n_cols; ++c) P.esize[c] = (int)f[PL_ESIZE0 + c];
    int carried = 0;
    for (int a = 0; a < NA; ++a) {
        if (val_cols[a].data == nullptr) {
            G.carried[a] = 0;
            G.const_cell[a] = const_cells[a];
            continue;
        }
        ++carried;
        if (carried > (int)f[PL_NCARRIED] || rx_esize(val_cols[a].kind) != (int)f[PL_ESIZE0 + kcols - 1 + carried]) {
            hs_set_error("hs_group_radix_run: value column %d does not match the plan", a);
            return HS_E_ARG;
        }
        P.src[kcols - 1 + carried] = val_cols[a].data;
        G.carried[a] = kcols - 1 + carried;
        G.val_kind[a] = val_cols[a].kind;
    }
    if (carried != (int)f[PL_NCARRIED]) {
        hs_set_error("hs_group_radix_run: %d travelling value columns, the plan has %d", carried, (int)f[PL_NCARRIED]);
        return HS_E_ARG;
    }

    auto pass = [&](const int64_t* seg_start, int64_t n_seg, int64_t* tile_base, int64_t max_tiles, int shift, int bits, bool first,
                    void* const* src, void* const* dst, int64_t* next_seg) -> int {
        P.seg_start = seg_start;
        P.tile_base = tile_base;
        P.n_seg = n_seg;
        P.shift = shift;
        P.bits = bits;
        P.first = first ? 1 : 0;
        if (!first)
            for (int c = 0; c < P.n_cols; ++c) P.src[c] = src[c];
        for (int c = 0; c < P.n_cols; ++c) P.dst[c] = dst[c];
        return rx_pass(stream, P, max_tiles, counters, scanned, scan_ws, n, next_seg);
    };
    int rc = pass(unit_bounds, n_units, tb0, f[PL_TILES1], 0, bits1, true, nullptr, buf_a, seg1);
    if (rc != HS_OK) return rc;
    void* const* tuples = buf_a;
    if (bits2) {
        rc = pass(seg1, f[PL_NSEG1], tb1, f[PL_TILES2], bits1, bits2, false, buf_a, buf_b, seg2);
        if (rc != HS_OK) return rc;
        tuples = buf_b;
    }

    const int64_t parts = f[PL_PARTS];
    G.seg_start = seg2;
    G.n_parts = parts;
    for (int c = 0; c < P.n_cols; ++c) {
        G.src[c] = tuples[c];
        G.esize[c] = P.esize[c];
    }
    G.spec = *spec;
    G.cap = (int)f[PL_CAP];
    G.quantise = (int)f[PL_QUANTISE];
    G.prov_key = (uint64_t*)(ws + f[PL_OFF_PKEY]);
    G.prov_key1 = G.prov_key + n;
    for (int a = 0; a < NA; ++a) G.prov_acc[a] = ws + f[PL_OFF_PACC] + (size_t)a * rx_align((size_t)n * f[PL_OSIZE]);
    G.pcount = (int64_t*)(ws + f[PL_OFF_PCOUNT]);
    G.flags = flags;
    static const bool stamps = getenv("HIPSPARK_RADIX_STAMPS") != nullptr;
    G.debug = stamps ? 1 : 0;
    int64_t* overflow = (int64_t*)(ws + f[PL_OFF_OVERFLOW]);  // [0] = count, [1 ..] = partitions
    int64_t* overflow2 = overflow + f[PL_PARTS] + 1;           // the same for the next table size
    hs_memset_async(overflow, 0, 8, stream);
    hs_memset_async(overflow2, 0, 8, stream);
    // every aggregate a SUM over an f32 / i32 column or an integer constant: the specialised fold (k_rx_fold_sum)
    int sum_cls = NA >= 1 && NA <= 3 ? 0 : -1;
    for (int a = 0; a < NA && sum_cls >= 0; ++a) {
        const bool is_int = spec->is_int[a] != 0;
        int c = -1;
        if (spec->op[a] != HS_AGG_SUM) c = -1;
        else if (G.carried[a] && G.val_kind[a] == HS_F32 && !is_int) c = 0;
        else if (G.carried[a] && G.val_kind[a] == HS_I32 && is_int) c = 1;
        else if (!G.carried[a] && is_int) c = 2;
        sum_cls = c < 0 ? -1 : (sum_cls | (c << (2 * a)));
    }
    if (stamps && !wide) sum_cls = -1;  // (the phase stamps live in the general fold)
    if (wide && sum_cls < 0) {
        hs_set_error("hs_group_radix_run: a wide STRING key needs the SUM-specialised fold");
        return HS_E_LIMIT;
    }
    const int km = wide ? kcols : (G.esize[0] == 4 ? 0 : 1), nc = (int)f[PL_NCARRIED];
    // todo: the partitions this launch works on (NULL: all), left: where it notes the ones that outgrow its tables
    auto fold = [&](int cap, int64_t* todo, int64_t* left) -> int {
        G.cap = cap;
        G.last = cap == (int)f[PL_CAP] ? 1 : 0;
        G.list = todo ? todo + 1 : nullptr;
        G.list_count = todo;
        G.overflow = left + 1;
        G.overflow_count = left;
        const size_t per_wave = rx_fold_words(cap, NA, wide != 0) * 8;
        int wpb = (int)(65536 / per_wave);
        wpb = wpb < 1 ? 1 : (wpb > 4 ? 4 : wpb);
        int64_t grid = (parts + wpb - 1) / wpb;
        if (grid > 256 * 32) grid = 256 * 32;
        RxFoldKernel kernel = nullptr;
        if (sum_cls >= 0 && sum_cls < RX_SUM_CODES && NA >= 1 && NA <= 3 && km >= 0 && km < RX_SUM_KM) kernel = RX_FOLD_SUM.k[NA - 1][sum_cls][km];
        if (!kernel) kernel = RX_FOLD[nc >= 0 && nc <= 4 ? nc : 5][cap <= 512 ? 0 : 1];
        hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(HS_WAVE * wpb), per_wave * wpb, stream, G);
        RX_CHECK_LAUNCH("hs_group_radix_run (fold)");
        return HS_OK;
    };
    // Three table sizes, smallest first: a partition is cut to hold ~half the LARGE table's slots in ROWS, and usually holds far
    // fewer distinct keys.  The fold is a chain of LDS round trips per 64-row step, one wave per partition - what it needs is
    // waves: 256-slot tables leave room for 28 per CU (512: 16), and a partition that outgrows 3/4 of a table moves to the next
    // size's list (round 4; 64 Mi rows / 4 Mi groups: fold 0.52 -> see profiles/r04_radix_tier_64M.txt).
    const int big = (int)f[PL_CAP], small = big > 512 ? 512 : big, tiny = small > 256 ? 256 : small;
    if (tiny < small) {
        rc = fold(tiny, nullptr, overflow);
        if (rc == HS_OK) rc = fold(small, overflow, overflow2);
        if (rc == HS_OK && small < big) rc = fold(big, overflow2, overflow2);
    } else if (small < big) {
        rc = fold(small, nullptr, overflow);
        if (rc == HS_OK) rc = fold(big, overflow, overflow);
    } else {
        rc = fold(big, nullptr, overflow);  // nothing can overflow into a list: a full table raises HS_FLAG_DICT_FULL ...
    }
    if (rc != HS_OK) return rc;
    int64_t* pscan = (int64_t*)(ws + f[PL_OFF_PSCAN]);
    rc = hs_exclusive_scan_i64(stream, G.pcount, parts, pscan, scan_ws);
    if (rc != HS_OK) return rc;
    hipLaunchKernelGGL(k_rx_unit_groups, dim3((unsigned)((n_units + 256) / 256)), dim3(256), 0, stream, (const int64_t*)pscan,
                       (int64_t)1 << (bits1 + bits2), (int32_t)n_units, out_unit_groups);
    RX_CHECK_LAUNCH("hs_group_radix_run (unit groups)");
    return HS_OK;
}

extern "C" int hs_group_radix_emit(void* stream_, const hs_radix_plan* plan, void* ws_, void* out_key, void* const* out_acc) {
    if (!plan || !ws_ || !out_key || (plan->f[PL_NA] > 0 && !out_acc)) {
        hs_set_error("hs_group_radix_emit: bad arguments");
        return HS_E_ARG;
    }
    const int64_t* f = plan->f;
    uint8_t* ws = (uint8_t*)ws_;
    RxEmit E;
    std::memset(&E, 0, sizeof(E));
    E.seg_start = (const int64_t*)(ws + (f[PL_BITS2] ? f[PL_OFF_SEG2] : f[PL_OFF_SEG1]));
    E.pscan = (const int64_t*)(ws + f[PL_OFF_PSCAN]);
    E.n_parts = f[PL_PARTS];
    E.prov_key = (const uint64_t*)(ws + f[PL_OFF_PKEY]);
    E.prov_key1 = E.prov_key + f[PL_N];
    E.n_acc = (int)f[PL_NA];
    E.osize = (int)f[PL_OSIZE];
    E.key_kind = (int)f[PL_KEYKIND];
    E.out_key = out_key;
    for (int a = 0; a < E.n_acc; ++a) {
        E.prov_acc[a] = ws + f[PL_OFF_PACC] + (size_t)a * rx_align((size_t)f[PL_N] * f[PL_OSIZE]);
        E.out_acc[a] = out_acc[a];
    }
    int64_t grid = (E.n_parts + 3) / 4;
    if (grid > 256 * 64) grid = 256 * 64;
    hipLaunchKernelGGL(k_rx_emit, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream_, E);
    RX_CHECK_LAUNCH("hs_group_radix_emit");
    return HS_OK;
}

/* debug (HIPSPARK_RADIX_STAMPS=1): cycles per phase of the fold kernel summed over waves since the last call:
 * [0] clear tables [1] wait for a chunk's loads [2] slot lookup [3] ranking [4] fold [5] emit [6] waves */
extern "C" int hs_group_radix_debug_stamps(uint64_t* out8) {
    unsigned long long zero[8] = {0};
    if (!out8 || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpyFromSymbol(out8, HIP_SYMBOL(rx_stamp_acc), sizeof(zero)) != hipSuccess ||
        hipMemcpyToSymbol(HIP_SYMBOL(rx_stamp_acc), zero, sizeof(zero)) != hipSuccess) {
        hs_set_error("hs_group_radix_debug_stamps failed");
        return HS_E_ARG;
    }
    return HS_OK;
}

// =====================================================================================================
// Merge order of a multi-rank final aggregate (reference: the shuffle files of a partition are read in block order,
// tasks.py:117-133): a STABLE sort of the partial rows by their order key (global block id, -1 = padding) with the
// same partition passes, least significant byte first.  Replaces torch.argsort on this path.
// =====================================================================================================
__global__ void __launch_bounds__(256) k_rx_iota(int64_t* out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = i;
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // the one segment of the passes: [0, n)
        out[n] = 0;
        out[n + 1] = n;
    }
}

extern "C" size_t hs_sort_by_order_ws_bytes(int64_t n) {
    const int64_t tiles = n / RX_TILE + 2;
    return rx_align((size_t)n * 8) * 2 + rx_align((size_t)(n + 2) * 8) + 256 + rx_align((size_t)(tiles << 8) * 8) +
           rx_align((size_t)((tiles << 8) + 1) * 8) + rx_align(hs_scan_ws_bytes(tiles << 8));
}

extern "C" int hs_sort_by_order(void* stream_, const int64_t* order, int64_t n, int64_t n_order, int64_t* out_perm,
                                int64_t* out_sorted, void* ws_) {
    if (n == 0) return HS_OK;
    if (!order || !out_perm || !out_sorted || !ws_ || n < 0 || n_order < 0) {
        hs_set_error("hs_sort_by_order: bad arguments");
        return HS_E_ARG;
    }
    hipStream_t stream = (hipStream_t)stream_;
    uint8_t* ws = (uint8_t*)ws_;
    const int64_t tiles = n / RX_TILE + 2;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        uint8_t* p = ws + off;
        off += rx_align(bytes);
        return p;
    };
    int64_t* key_b = (int64_t*)take((size_t)n * 8);
    int64_t* perm_b = (int64_t*)take((size_t)n * 8);
    int64_t* iota = (int64_t*)take((size_t)(n + 2) * 8);  // [n], then the segment bounds {0, n}
    int64_t* tile_base = (int64_t*)take(256);
    int64_t* counters = (int64_t*)take((size_t)(tiles << 8) * 8);
    int64_t* scanned = (int64_t*)take((size_t)((tiles << 8) + 1) * 8);
    void* scan_ws = take(hs_scan_ws_bytes(tiles << 8));
    hipLaunchKernelGGL(k_rx_iota, dim3((unsigned)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256)), dim3(256), 0, stream, iota, n);
    RX_CHECK_LAUNCH("hs_sort_by_order (iota)");
    int bits = 1;
    while (bits < 64 && ((int64_t)1 << bits) <= n_order) ++bits;  // values + 1 lie in [0, n_order]
    const int passes = (bits + 7) / 8;
    RxPass P;
    std::memset(&P, 0, sizeof(P));
    P.seg_start = iota + n;
    P.tile_base = tile_base;
    P.n_seg = 1;
    P.n_cols = 2;
    P.esize[0] = P.esize[1] = 8;
    P.mode = RX_BIN_PLUS1;
    for (int k = 0; k < passes; ++k) {
        const bool to_out = ((passes - 1 - k) & 1) == 0;  // the last pass lands in the caller's arrays
        P.first = k == 0 ? 1 : 0;
        P.key = hs_col{HS_I64, -1, order, nullptr, nullptr};
        P.sel = nullptr;
        P.row0 = 0;
        P.src[0] = k == 0 ? nullptr : (to_out ? (const void*)key_b : (const void*)out_sorted);
        P.src[1] = k == 0 ? (const void*)iota : (to_out ? (const void*)perm_b : (const void*)out_perm);
        P.dst[0] = to_out ? (void*)out_sorted : (void*)key_b;
        P.dst[1] = to_out ? (void*)out_perm : (void*)perm_b;
        P.shift = 8 * k;
        P.bits = bits - 8 * k < 8 ? bits - 8 * k : 8;
        const int rc = rx_pass(stream, P, tiles, counters, scanned, scan_ws, n, nullptr);
        if (rc != HS_OK) return rc;
    }
    return HS_OK;
}

// =====================================================================================================
// ORDER BY / LIMIT over result rows (include/hipspark.h hs_order_by; the reference has no ordering).
//
// Every key column becomes a run of bytes whose unsigned order is the wanted order; the runs of all keys, one after the
// other, are the row's sort key, cut into 64-bit words (byte 0 of the key = most significant byte of word 0).  The words
// are sorted least significant first with the stable partition passes above (raw = 2: the bin is a byte of the word),
// carrying (word, row): k_ob_keys forms ONE word per launch - for rows in place (coalesced) when it is the first word to
// be sorted, through the row list the earlier words left behind otherwise, which is the gather any multi-word LSD sort
// pays - so the workspace does not grow with the key's length.  The kernel also folds the AND and the OR of its words: a
// byte in which they agree is the same in every row, its histogram would have one occupied bin, and its pass is skipped
// (timestamps, small integers, string padding, the unused tail of the last word).
//
// 0 <= limit < rows: k_ob_select / k_ob_pick walk the first word's bytes, most significant first, with one 256-bin
// histogram of the rows that still match the prefix - nothing is moved - until the limit-th smallest word is known;
// k_ob_count / k_ob_compact keep the rows at or below it, in input order (ballot ranks inside a wave, a scan over the
// tiles: no atomics decide a position), and only those rows are sorted.  Rows beyond the cut that tie with it on the first
// word stay candidates, so the first `limit` rows of the candidates' stable sort are those of the full one.
// =====================================================================================================
constexpr int OB_THREADS = 256;
constexpr int OB_WAVES = OB_THREADS / HS_WAVE;
constexpr int OB_STEPS = 8;                              // 64-row steps a wave ranks in the compaction
constexpr int OB_TILE = OB_THREADS * OB_STEPS;           // 2048 rows
constexpr int OB_MAX_PARTS = 8;                          // a word has 8 bytes: at most 8 keys meet in it

struct ObPart {
    int32_t key, off, nbytes, pos;  // bytes [off, off + nbytes) of the key's run are bytes [pos, pos + nbytes) of the word (0 = most significant)
};
struct ObKeys {
    hs_col col[HS_MAX_COLS];
    int32_t width[HS_MAX_COLS];    // bytes of the key's run
    int32_t str_cap[HS_MAX_COLS];  // HS_STR: bytes of the (zero-padded) string; width = str_cap + 1 when a length byte follows
    int32_t desc[HS_MAX_COLS];
    ObPart part[OB_MAX_PARTS];
    int32_t n_parts, first;        // first: the launch also writes out_rows and the passes' one segment {0, n}
    const int64_t* rows;           // the rows in their present order (null: position = row)
    int64_t n;
    uint64_t* out_words;
    int64_t* out_rows;
    unsigned long long* and_or;    // [2]: AND and OR of all words
    int64_t* seg;
};
static_assert(sizeof(ObKeys) % 8 == 0, "ObKeys");

// the bits of a FLOAT cell as an unsigned word whose order is the cell's order (also the MIN / MAX accumulator of
// hs_window_agg, which turns the winning word back into bits)
__device__ __forceinline__ uint32_t ob_f32_word(uint32_t b) {
    if ((b & 0x7fffffffu) > 0x7f800000u) b = 0x7fc00000u;  // every NaN: one value, after +inf
    if (b == 0x80000000u) b = 0u;                          // -0.0 == +0.0
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// a numeric cell as an unsigned number of the column's width whose order is the cell's order
__device__ __forceinline__ uint64_t ob_numeric(const hs_col& c, int64_t row) {
    switch (c.kind) {
        case HS_I32: return (uint64_t)(((const uint32_t*)c.data)[row] ^ 0x80000000u);
        case HS_I64: return ((const uint64_t*)c.data)[row] ^ 0x8000000000000000ull;
        case HS_F32: return (uint64_t)ob_f32_word(((const uint32_t*)c.data)[row]);
        case HS_F64: {
            uint64_t b = ((const uint64_t*)c.data)[row];
            if ((b & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) b = 0x7ff8000000000000ull;
            if (b == 0x8000000000000000ull) b = 0ull;
            return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
        }
        default: return (uint64_t)((const uint8_t*)c.data)[row];  // HS_U8
    }
}

// bytes [off, off + nbytes) of key k's run (which starts at byte `at` of the row's key) that fall into word w: one
// layout rule for the host, which lists a word's parts for k_ob_keys, and for k_distinct_heads, which walks every word
__host__ __device__ inline bool ob_part_of(int32_t k, int64_t at, int32_t width, int32_t w, ObPart& out) {
    const int64_t b = at > (int64_t)w * 8 ? at : (int64_t)w * 8;
    const int64_t e = at + width < (int64_t)(w + 1) * 8 ? at + width : (int64_t)(w + 1) * 8;
    if (b >= e) return false;
    out = ObPart{k, (int32_t)(b - at), (int32_t)(e - b), (int32_t)(b - (int64_t)w * 8)};
    return true;
}

// one part of a row's key word, in its place in the word: the encoding of every key type (k_ob_keys ORs the parts of
// one word; k_distinct_heads re-forms the words of two rows with it, so its equality IS the sort's)
__device__ __forceinline__ uint64_t ob_part_bits(const ObKeys& A, const ObPart part, int64_t row) {
    const hs_col& c = A.col[part.key];
    const uint64_t mask = part.nbytes == 8 ? ~0ull : (1ull << (8 * part.nbytes)) - 1ull;
    uint64_t chunk = 0;
    if (c.kind == HS_STR) {
        const HsStr s = hs_str_at(c, row);
        const uint32_t cap = (uint32_t)A.str_cap[part.key];
        for (uint32_t j = (uint32_t)part.off; j < (uint32_t)(part.off + part.nbytes); ++j)
            chunk = (chunk << 8) | (uint64_t)(j < cap ? (j < s.len ? s.p[j] : 0u) : s.len);
    } else {
        chunk = (ob_numeric(c, row) >> (8 * (A.width[part.key] - part.off - part.nbytes))) & mask;
    }
    if (A.desc[part.key]) chunk ^= mask;
    return chunk << (8 * (8 - part.pos - part.nbytes));
}

__global__ void __launch_bounds__(OB_THREADS) k_ob_keys(const ObKeys A_kernarg) {
    HS_KERNARG(ObKeys, A);
    const int lane = threadIdx.x & (HS_WAVE - 1);
    unsigned long long all_and = ~0ull, all_or = 0ull;
    for (int64_t i = (int64_t)blockIdx.x * OB_THREADS + threadIdx.x; i < A.n; i += (int64_t)gridDim.x * OB_THREADS) {
        const int64_t row = A.rows ? A.rows[i] : i;
        uint64_t word = 0;
        for (int p = 0; p < A.n_parts; ++p) word |= ob_part_bits(A, A.part[p], row);
        A.out_words[i] = word;
        if (A.first) A.out_rows[i] = row;
        all_and &= word;
        all_or |= word;
    }
    for (int d = HS_WAVE / 2; d > 0; d >>= 1) {
        all_and &= __shfl_xor(all_and, d, HS_WAVE);
        all_or |= __shfl_xor(all_or, d, HS_WAVE);
    }
    if (lane == 0) {  // two folds per wave of a grid of at most 1024 workgroups; no position depends on them
        atomicAnd(&A.and_or[0], all_and);
        atomicOr(&A.and_or[1], all_or);
    }
    if (A.first && blockIdx.x == 0 && threadIdx.x == 0) {
        A.seg[0] = 0;
        A.seg[1] = A.n;
    }
}

__global__ void __launch_bounds__(OB_THREADS) k_ob_iota(int64_t* out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * OB_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * OB_THREADS) out[i] = i;
}

// the longest string of a variable-length column
__global__ void __launch_bounds__(OB_THREADS) k_ob_maxlen(const uint8_t* lens, int64_t n, uint32_t* out) {
    uint32_t m = 0;
    for (int64_t i = (int64_t)blockIdx.x * OB_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * OB_THREADS)
        m = lens[i] > m ? lens[i] : m;
    for (int d = HS_WAVE / 2; d > 0; d >>= 1) {
        const uint32_t o = __shfl_xor(m, d, HS_WAVE);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & (HS_WAVE - 1)) == 0 && m) atomicMax(out, m);
}

// selection state: the bytes of the limit-th smallest first word found so far
struct ObSelect {
    uint64_t prefix, mask;  // rows still in the race: (word & mask) == prefix
    int64_t k;              // the word looked for is the k-th smallest (1-based) among them
};

// one round of the radix select: histogram of byte `shift / 8` over the rows that match the prefix.  Nothing is moved.
__global__ void __launch_bounds__(OB_THREADS) k_ob_select(const uint64_t* words, int64_t n, const ObSelect* state, int shift,
                                                          unsigned long long* hist) {
    __shared__ uint32_t s_hist[OB_WAVES][256];  // one per wave: LDS atomics of different waves never meet
    const int tid = threadIdx.x, w = tid / HS_WAVE;
    for (int i = tid; i < OB_WAVES * 256; i += OB_THREADS) s_hist[i >> 8][i & 255] = 0;
    __syncthreads();
    const uint64_t prefix = state->prefix, mask = state->mask;
    for (int64_t i = (int64_t)blockIdx.x * OB_THREADS + tid; i < n; i += (int64_t)gridDim.x * OB_THREADS) {
        const uint64_t word = words[i];
        if ((word & mask) == prefix) atomicAdd(&s_hist[w][(uint32_t)(word >> shift) & 0xffu], 1u);
    }
    __syncthreads();
    uint32_t total = 0;
#pragma unroll
    for (int k = 0; k < OB_WAVES; ++k) total += s_hist[k][tid];
    if (total) atomicAdd(&hist[tid], (unsigned long long)total);  // a count, not a rank: the order of the adds is immaterial
}

// ... and the bin that holds the k-th row: its byte joins the prefix.  One workgroup; clears the histogram for the next round.
__global__ void __launch_bounds__(256) k_ob_pick(ObSelect* state, int shift, unsigned long long* hist) {
    __shared__ int64_t s_wave[4];
    const int tid = threadIdx.x, lane = tid & (HS_WAVE - 1), w = tid / HS_WAVE;
    const int64_t mine = (int64_t)hist[tid];
    hist[tid] = 0;
    int64_t x = mine;
    for (int d = 1; d < HS_WAVE; d <<= 1) {
        const int64_t up = __shfl_up(x, d, HS_WAVE);
        if (lane >= d) x += up;
    }
    if (lane == HS_WAVE - 1) s_wave[w] = x;
    const int64_t k = state->k;
    const uint64_t prefix = state->prefix, mask = state->mask;
    __syncthreads();
    for (int j = 0; j < w; ++j) x += s_wave[j];
    if (x - mine < k && k <= x) {  // exactly one bin
        state->prefix = prefix | ((uint64_t)tid << shift);
        state->mask = mask | (0xffull << shift);
        state->k = k - (x - mine);
    }
}

// rows whose first word is at or below the selected one, per tile ...
__global__ void __launch_bounds__(OB_THREADS) k_ob_count(const uint64_t* words, int64_t n, const ObSelect* state, int64_t* counts) {
    __shared__ uint32_t s_cnt[OB_WAVES];
    const int lane = threadIdx.x & (HS_WAVE - 1), w = threadIdx.x / HS_WAVE;
    const uint64_t cut = state->prefix;
    const int64_t first = (int64_t)blockIdx.x * OB_TILE + (int64_t)w * (OB_STEPS * HS_WAVE) + lane;
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < OB_STEPS; ++j) {
        const int64_t i = first + j * HS_WAVE;
        c += (uint32_t)__popcll(__ballot(i < n && words[i] <= cut));
    }
    if (lane == 0) s_cnt[w] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = (int64_t)s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}
// ... and their row numbers in input order: the tile's scanned count, the waves before mine, the steps before this one,
// the lanes below me
__global__ void __launch_bounds__(OB_THREADS) k_ob_compact(const uint64_t* words, int64_t n, const ObSelect* state,
                                                           const int64_t* start, int64_t* out_rows) {
    __shared__ uint32_t s_cnt[OB_WAVES];
    const int lane = threadIdx.x & (HS_WAVE - 1), w = threadIdx.x / HS_WAVE;
    const uint64_t cut = state->prefix;
    const int64_t first = (int64_t)blockIdx.x * OB_TILE + (int64_t)w * (OB_STEPS * HS_WAVE) + lane;
    uint64_t bal[OB_STEPS];
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < OB_STEPS; ++j) {
        const int64_t i = first + j * HS_WAVE;
        bal[j] = __ballot(i < n && words[i] <= cut);
        c += (uint32_t)__popcll(bal[j]);
    }
    if (lane == 0) s_cnt[w] = c;
    __syncthreads();
    int64_t at = start[blockIdx.x];
    for (int j = 0; j < w; ++j) at += s_cnt[j];
    const uint64_t below = (1ull << lane) - 1ull;
#pragma unroll
    for (int j = 0; j < OB_STEPS; ++j) {
        if ((bal[j] >> lane) & 1ull) out_rows[at + __popcll(bal[j] & below)] = first + j * HS_WAVE;
        at += __popcll(bal[j]);
    }
}

static_assert(OB_WAVES == 4, "k_ob_count adds four wave counts");

static unsigned ob_grid(int64_t n) {
    const int64_t g = (n + OB_THREADS - 1) / OB_THREADS;
    return (unsigned)(g > 1024 ? 1024 : (g < 1 ? 1 : g));
}

extern "C" size_t hs_order_by_ws_bytes(int64_t nrows, int32_t n_keys, int32_t max_key_words) {
    (void)n_keys;
    (void)max_key_words;
    if (nrows < 0) return 0;
    const int64_t tiles = nrows / RX_TILE + 2;
    return rx_align((size_t)nrows * 8) * 4 + 256 + 256 + rx_align(256 * 8) + rx_align((size_t)(tiles << 8) * 8) +
           rx_align((size_t)((tiles << 8) + 1) * 8) + rx_align(hs_scan_ws_bytes(tiles << 8));
}

static bool ob_kind_ok(const hs_col& c) {
    switch (c.kind) {
        case HS_I32:
        case HS_F32:
        case HS_I64:
        case HS_F64:
        case HS_U8: return c.data != nullptr;
        case HS_STR: return c.fixed_len == 0 || (c.data && c.fixed_len <= 255 && (c.fixed_len > 0 || (c.lens && c.offs)));
        default: return false;
    }
}

// What every entry over ob_sort refuses of its key columns, under its own name and in its own nouns: before its
// `nrows == 0` return the limit (`many`: "keys" / "columns" / "partition and order columns") and a narrow column, behind
// it a column ob_kind_ok does not take (`one` / `done`: "key" ... "ordered" / "column" ... "compared").
static int ob_refuse_keys(const char* name, const hs_col* keys, int32_t n_keys, const char* many) {
    if (n_keys > HS_MAX_COLS) {
        hs_set_error("%s: more than %d %s", name, HS_MAX_COLS, many);
        return HS_E_LIMIT;
    }
    return hs_refuse_narrow(name, keys, n_keys) ? HS_E_ARG : HS_OK;
}
static int ob_refuse_kinds(const char* name, const hs_col* keys, int32_t n_keys, const char* one, const char* done) {
    for (int k = 0; k < n_keys; ++k)
        if (!ob_kind_ok(keys[k])) {
            hs_set_error("%s: %s %d is not a column that can be %s", name, one, k, done);
            return HS_E_ARG;
        }
    return HS_OK;
}

// a launch inside ob_sort: the error names the entry point that called
#define OB_CHECK_LAUNCH(what)                                        \
    if (hipGetLastError() != hipSuccess) {                           \
        hs_set_error("%s (" what "): kernel launch failed", name);   \
        return HS_E_LAUNCH;                                          \
    }

// what the sort leaves behind for its callers
struct ObSorted {
    ObKeys keys;          // col / width / str_cap / desc as the sort used them
    int32_t n_words;      // 64-bit words of a row's key
    int64_t n, count;     // rows = min(nrows, *nrows_dev); rows of the answer = min(rows, limit)
    const int64_t* rows;  // the answer's rows in order (in the workspace); null: the rows in place (the keys have no byte)
    size_t ws_bytes;      // bytes of the workspace the sort laid out: what follows them is the caller's
    const uint64_t* words;  // word 0 of the answer's rows, in their order (null with `rows`)
    uint64_t varying;     // `unsorted`: the bits of the first word formed that differ between rows
    int32_t unsorted;     // `dense` ended the sort before any pass moved a row: `rows` / `words` stand in input order
};

// The sorted rows as the kernels that look for the runs of equal keys take them: the first members of DhArgs
// (k_distinct_heads) and of WinHeads (k_win_heads)
struct ObRun {
    ObKeys K;               // col / width / str_cap / desc of the sort
    int32_t n_keys, n_words;
    const int64_t* perm;    // the rows, sorted by all keys (null: position = row, the keys have no byte)
    const uint64_t* words;  // a key of ONE word: that word of the sorted rows, as the sort left it - compared instead of
                            // formed again (null: the words are formed from the columns)
    int64_t n;
};
static ObRun ob_run(const ObSorted& S, int32_t n_keys) {
    // one word per row: the sorted words ARE the rows' keys
    return ObRun{S.keys, n_keys, S.n_words, S.rows, S.n_words == 1 && S.rows ? S.words : nullptr, S.n};
}

// hs_mark_first's dense path holds a key of ONE word whose varying bits are few (defined with its kernels, below)
static bool mf_dense_fits(int32_t n_words, uint64_t varying);
enum { OB_SORT = 0, OB_DENSE_IF_FITS = 1, OB_DENSE_ONLY = 2 };  // ob_sort's `dense`

// The sort of hs_order_by, shared with hs_distinct and hs_mark_first: checked arguments in, *out_count (HOST) and `S`
// out.  nrows > 0, limit != 0, 0 <= n_keys <= HS_MAX_COLS, every key ob_kind_ok.  `name`: the calling entry point, for
// the error texts.  `in_rows` (device, n_in of them, each below nrows; limit < 0 and no nrows_dev with it): only these
// rows are sorted, in the order they are listed - the list the LIMIT path hands sort_rows, given by the caller.
// `dense` (hs_mark_first alone): OB_DENSE_IF_FITS returns after the first word is formed, before any pass, when the key
// fits the dense path (S.unsorted); OB_DENSE_ONLY returns there whatever the key, and the caller refuses what does not fit.
static int ob_sort(hipStream_t stream, const hs_col* keys, const int32_t* descending, int32_t n_keys, int64_t nrows,
                   const int64_t* nrows_dev, int64_t limit, int64_t* out_count, void* ws_, const char* name, ObSorted& S,
                   const int64_t* in_rows = nullptr, int64_t n_in = 0, int dense = OB_SORT) {
    std::memset(&S, 0, sizeof(S));
    uint8_t* ws = (uint8_t*)ws_;
    const int64_t tiles_max = nrows / RX_TILE + 2;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        uint8_t* p = ws + off;
        off += rx_align(bytes);
        return p;
    };
    uint64_t* K[2];
    int64_t* R[2];
    K[0] = (uint64_t*)take((size_t)nrows * 8);
    K[1] = (uint64_t*)take((size_t)nrows * 8);
    R[0] = (int64_t*)take((size_t)nrows * 8);
    R[1] = (int64_t*)take((size_t)nrows * 8);
    unsigned long long* state = (unsigned long long*)take(256);  // [0] AND, [1] OR, [2..4] ObSelect, [5] longest string, [6..7] segment
    int64_t* tile_base = (int64_t*)take(256);
    unsigned long long* hist = (unsigned long long*)take(256 * 8);
    int64_t* counters = (int64_t*)take((size_t)(tiles_max << 8) * 8);
    int64_t* scanned = (int64_t*)take((size_t)((tiles_max << 8) + 1) * 8);
    void* scan_ws = take(hs_scan_ws_bytes(tiles_max << 8));
    S.ws_bytes = off;
    ObSelect* select = (ObSelect*)(state + 2);
    int64_t* seg = (int64_t*)(state + 6);

    auto read_back = [&](void* host, const void* dev, size_t bytes) {
        return hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, stream) == hipSuccess &&
               hipStreamSynchronize(stream) == hipSuccess;
    };
    int64_t n = nrows;
    if (nrows_dev) {
        int64_t exact = 0;
        if (!read_back(&exact, nrows_dev, 8)) {
            hs_set_error("%s: reading the row count failed", name);
            return HS_E_LAUNCH;
        }
        n = exact < n ? (exact < 0 ? 0 : exact) : n;
    }
    const int64_t cells = n;  // rows of the columns: a variable-length key's longest string is looked for among all of them
    if (in_rows) n = n_in;
    const int64_t count = limit < 0 || limit > n ? n : limit;
    *out_count = count;
    S.n = n;
    S.count = count;
    if (count == 0) return HS_OK;

    // the key's layout: widths of the runs, then the parts of every word
    ObKeys& A = S.keys;
    int64_t total_bytes = 0;
    for (int k = 0; k < n_keys; ++k) {
        const hs_col& c = keys[k];
        A.col[k] = c;
        A.desc[k] = descending[k] ? 1 : 0;
        if (c.kind == HS_STR && c.fixed_len < 0) {
            hs_memset_async(state + 5, 0, 8, stream);
            hipLaunchKernelGGL(k_ob_maxlen, dim3(ob_grid(cells)), dim3(OB_THREADS), 0, stream, c.lens, cells, (uint32_t*)(state + 5));
            OB_CHECK_LAUNCH("longest string");
            uint32_t longest = 0;
            if (!read_back(&longest, state + 5, 4)) {
                hs_set_error("%s: reading the longest string failed", name);
                return HS_E_LAUNCH;
            }
            A.str_cap[k] = (int32_t)longest;
            A.width[k] = (int32_t)longest + 1;  // the length byte: a prefix sorts before its extensions
        } else if (c.kind == HS_STR) {
            A.str_cap[k] = A.width[k] = c.fixed_len;  // one length: no tie left to break
        } else {
            A.width[k] = rx_esize(c.kind);
        }
        total_bytes += A.width[k];
    }
    const int n_words = (int)((total_bytes + 7) / 8);
    S.n_words = n_words;
    if (n_words == 0) return HS_OK;

    // word w of `m` rows (in place, or those of `rows`) -> out_words; -> the bytes of the word that differ between rows
    auto form = [&](int w, const int64_t* rows, int64_t m, uint64_t* out_words, int64_t* out_rows, uint64_t& and_bits,
                    uint64_t& varying) {
        A.n_parts = 0;
        int64_t at = 0;
        for (int k = 0; k < n_keys; ++k) {
            ObPart part;
            if (ob_part_of(k, at, A.width[k], w, part)) A.part[A.n_parts++] = part;
            at += A.width[k];
        }
        A.rows = rows;
        A.n = m;
        A.out_words = out_words;
        A.out_rows = out_rows;
        A.first = out_rows ? 1 : 0;
        A.and_or = state;
        A.seg = seg;
        hs_memset_async(state, 0xff, 8, stream);
        hs_memset_async(state + 1, 0, 8, stream);
        hipLaunchKernelGGL(k_ob_keys, dim3(ob_grid(m)), dim3(OB_THREADS), 0, stream, A);
        OB_CHECK_LAUNCH("key words");
        unsigned long long ao[2] = {0, 0};
        if (!read_back(ao, state, 16)) {
            hs_set_error("%s: reading the key summary failed", name);
            return HS_E_LAUNCH;
        }
        and_bits = ao[0];
        varying = ao[0] ^ ao[1];
        return HS_OK;
    };
    // stable sort of m rows (in place, or the list `rows`, which may be K[1]) by all words -> the buffer that holds them
    auto sort_rows = [&](const int64_t* rows, int64_t m, const int64_t*& sorted) {
        int cur = 0;
        RxPass P;
        std::memset(&P, 0, sizeof(P));
        P.seg_start = seg;
        P.tile_base = tile_base;
        P.n_seg = 1;
        P.n_cols = 2;
        P.esize[0] = P.esize[1] = 8;
        P.mode = RX_BIN_VALUE;
        P.bits = 8;
        const int64_t tiles = m / RX_TILE + 2;
        for (int w = n_words - 1; w >= 0; --w) {
            const bool first = w == n_words - 1;
            uint64_t and_bits = 0, varying = 0;
            int rc = form(w, first ? rows : R[cur], m, K[cur], first ? R[cur] : nullptr, and_bits, varying);
            if (rc != HS_OK) return rc;
            if (first && (dense == OB_DENSE_ONLY || (dense == OB_DENSE_IF_FITS && mf_dense_fits(n_words, varying)))) {
                S.unsorted = 1;
                S.varying = varying;
                break;
            }
            for (int b = 0; b < 8; ++b) {
                if (((varying >> (8 * b)) & 0xffull) == 0) continue;  // one occupied bin: the pass would move nothing
                P.src[0] = K[cur];
                P.src[1] = R[cur];
                P.dst[0] = K[cur ^ 1];
                P.dst[1] = R[cur ^ 1];
                P.shift = 8 * b;
                rc = rx_pass(stream, P, tiles, counters, scanned, scan_ws, m, nullptr);
                if (rc != HS_OK) return rc;
                cur ^= 1;
            }
        }
        sorted = R[cur];
        S.words = K[cur];  // word 0 was formed last and travelled with the rows
        return HS_OK;
    };

    const int64_t* sorted = nullptr;
    if (count == n) {
        const int rc = sort_rows(in_rows, n, sorted);
        if (rc != HS_OK) return rc;
    } else {
        // the count-th smallest first word, then the rows at or below it
        uint64_t and_bits = 0, varying = 0;
        int rc = form(0, nullptr, n, K[0], nullptr, and_bits, varying);
        if (rc != HS_OK) return rc;
        ObSelect init{0, 0, count};
        for (int b = 0; b < 8; ++b)
            if (((varying >> (8 * b)) & 0xffull) == 0) init.mask |= 0xffull << (8 * b);
        init.prefix = and_bits & init.mask;
        if (hipMemcpyAsync(select, &init, sizeof(init), hipMemcpyHostToDevice, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess) {  // `init` leaves scope
            hs_set_error("%s: writing the selection state failed", name);
            return HS_E_LAUNCH;
        }
        hs_memset_async(hist, 0, 256 * 8, stream);
        for (int b = 7; b >= 0; --b) {
            if ((init.mask >> (8 * b)) & 0xffull) continue;
            hipLaunchKernelGGL(k_ob_select, dim3(ob_grid(n)), dim3(OB_THREADS), 0, stream, (const uint64_t*)K[0], n,
                               (const ObSelect*)select, 8 * b, hist);
            hipLaunchKernelGGL(k_ob_pick, dim3(1), dim3(256), 0, stream, select, 8 * b, hist);
            OB_CHECK_LAUNCH("select");
        }
        const int64_t nct = (n + OB_TILE - 1) / OB_TILE;
        hipLaunchKernelGGL(k_ob_count, dim3((unsigned)nct), dim3(OB_THREADS), 0, stream, (const uint64_t*)K[0], n,
                           (const ObSelect*)select, counters);
        OB_CHECK_LAUNCH("count");
        rc = hs_exclusive_scan_i64(stream, counters, nct, scanned, scan_ws);
        if (rc != HS_OK) return rc;
        hipLaunchKernelGGL(k_ob_compact, dim3((unsigned)nct), dim3(OB_THREADS), 0, stream, (const uint64_t*)K[0], n,
                           (const ObSelect*)select, (const int64_t*)scanned, (int64_t*)K[1]);
        OB_CHECK_LAUNCH("compact");
        int64_t candidates = 0;
        if (!read_back(&candidates, scanned + nct, 8) || candidates < count || candidates > n) {
            hs_set_error("%s: the selection kept %lld rows of %lld for a limit of %lld", name, (long long)candidates,
                         (long long)n, (long long)count);
            return HS_E_LAUNCH;
        }
        rc = sort_rows((const int64_t*)K[1], candidates, sorted);
        if (rc != HS_OK) return rc;
    }
    S.rows = sorted;
    return HS_OK;
}

extern "C" int hs_order_by(void* stream_, const hs_col* keys, const int32_t* descending, int32_t n_keys, int64_t nrows,
                           const int64_t* nrows_dev, int64_t limit, int64_t* out_perm, int64_t* out_count, void* ws_,
                           uint32_t* flags) {
    (void)flags;
    if (n_keys < 0 || nrows < 0 || !out_perm || !out_count || !ws_ || (n_keys > 0 && (!keys || !descending)) ||
        (n_keys == 0 && limit < 0)) {
        hs_set_error("hs_order_by: bad arguments");
        return HS_E_ARG;
    }
    int rc = ob_refuse_keys("hs_order_by", keys, n_keys, "keys");
    if (rc != HS_OK) return rc;
    *out_count = 0;
    if (nrows == 0 || limit == 0) return HS_OK;
    if ((rc = ob_refuse_kinds("hs_order_by", keys, n_keys, "key", "ordered")) != HS_OK) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    ObSorted S;
    rc = ob_sort(stream, keys, descending, n_keys, nrows, nrows_dev, limit, out_count, ws_, "hs_order_by", S);
    if (rc != HS_OK || S.count == 0) return rc;
    if (!S.rows) {
        hipLaunchKernelGGL(k_ob_iota, dim3(ob_grid(S.count)), dim3(OB_THREADS), 0, stream, out_perm, S.count);
        RX_CHECK_LAUNCH("hs_order_by (rows in place)");
        return HS_OK;
    }
    if (hipMemcpyAsync(out_perm, S.rows, (size_t)S.count * 8, hipMemcpyDeviceToDevice, stream) != hipSuccess) {
        hs_set_error("hs_order_by: copying the row list failed");
        return HS_E_LAUNCH;
    }
    return HS_OK;
}

// =====================================================================================================
// SELECT DISTINCT over result rows (include/hipspark.h hs_distinct; the reference has no DISTINCT).
//
// Rows are equal iff all their key words are equal, the words being hs_order_by's.  ob_sort orders the rows by every key,
// ascending: equal rows become neighbours and, the sort being stable, stand in input order, so the first row of a run of
// equal rows - its HEAD - is the run's smallest input row.  k_distinct_heads marks the heads in INPUT order
// (keep[perm[j]] = 1 iff j == 0 or row perm[j] differs from row perm[j - 1] in some word) and hs_compact turns the mask
// into the ascending list of surviving rows: no second sort.  The sort keeps one word per row at a time, so the words of
// both rows are formed again, with ob_part_bits: a lane forms its own row's word and takes its left neighbour's through a
// wave shuffle; lane 0, whose neighbour belongs to the previous wave step or to the previous workgroup's tile, loads
// that row from the list and forms its word itself.  A key of ONE word (one INTEGER, two INTEGERs, a code and an
// INTEGER) needs none of that: the sorted words the sort leaves behind are the rows' keys, read coalesced.  No LDS, no
// atomics; the pass is bound by the gathers of the key cells (one per row and word) and the byte scattered into keep.
// =====================================================================================================
struct DhArgs : ObRun {
    uint8_t* keep;        // [n], input order
    int32_t* mark;        // hs_mark_first: INTEGER cells, input order, instead of `keep` (rows outside perm are not written)
};
static_assert(sizeof(DhArgs) == sizeof(ObRun) + 16, "DhArgs");  // `keep` directly behind the base: see WinHeads

// word w of a row's key, formed again from the columns (k_distinct_heads, k_win_heads)
__device__ __forceinline__ uint64_t ob_word(const ObKeys& K, int32_t n_keys, int32_t w, int64_t row) {
    uint64_t word = 0;
    int64_t at = 0;
    for (int k = 0; k < n_keys; ++k) {
        ObPart part;
        if (ob_part_of(k, at, K.width[k], w, part)) word |= ob_part_bits(K, part, row);
        at += K.width[k];
    }
    return word;
}
__device__ __forceinline__ uint64_t dh_word(const DhArgs& A, int32_t w, int64_t row) { return ob_word(A.K, A.n_keys, w, row); }

__global__ void __launch_bounds__(OB_THREADS) k_distinct_heads(const DhArgs A_kernarg) {
    HS_KERNARG(DhArgs, A);
    const int lane = threadIdx.x & (HS_WAVE - 1), wave = threadIdx.x / HS_WAVE;
    const int64_t first = (int64_t)blockIdx.x * OB_TILE + (int64_t)wave * (OB_STEPS * HS_WAVE) + lane;
    for (int j = 0; j < OB_STEPS; ++j) {
        const int64_t i = first + j * HS_WAVE;
        if (i - lane >= A.n) break;                   // the whole wave step lies past the rows
        const bool live = i < A.n;
        const int64_t pos = live ? i : A.n - 1;       // lanes past the end repeat the last row: every read stays inside
        const int64_t row = A.perm ? A.perm[pos] : pos;
        // lane 0's left neighbour sits in no lane of this step: sorted position i - 1, loaded explicitly
        const int64_t before = (lane == 0 && i > 0) ? (A.perm ? A.perm[i - 1] : i - 1) : row;
        bool differs = false;
        if (A.words) {  // coalesced: the sort's own words, no gather from the columns
            const unsigned long long mine = A.words[pos];
            unsigned long long left = __shfl_up(mine, 1, HS_WAVE);
            if (lane == 0 && i > 0) left = A.words[i - 1];
            differs = mine != left;
        } else for (int32_t w = 0; w < A.n_words; ++w) {
            const unsigned long long mine = dh_word(A, w, row);
            unsigned long long left = __shfl_up(mine, 1, HS_WAVE);
            if (lane == 0) left = dh_word(A, w, before);
            differs |= mine != left;
            if (__ballot(!differs) == 0) break;       // every lane of the step has found its difference
        }
        if (live) {
            const int head = (i == 0 || differs) ? 1 : 0;
            if (A.mark) A.mark[row] = head;
            else A.keep[row] = (uint8_t)head;
        }
    }
}

extern "C" int hs_compact(void* stream, const uint8_t* mask, int64_t nrows, int64_t* sel, int64_t* count, void* ws);

extern "C" size_t hs_distinct_ws_bytes(int64_t nrows, int32_t n_keys, int32_t max_key_words) {
    if (nrows < 0) return 0;
    // the sort's workspace, then the keep mask, the device count and the compaction's scan workspace
    return hs_order_by_ws_bytes(nrows, n_keys, max_key_words) + rx_align((size_t)nrows) + 256 + rx_align(hs_scan_ws_bytes(nrows));
}

extern "C" int hs_distinct(void* stream_, const hs_col* keys, int32_t n_keys, int64_t nrows, const int64_t* nrows_dev,
                           int64_t* out_perm, int64_t* out_count, void* ws_, uint32_t* flags) {
    (void)flags;
    if (n_keys <= 0 || nrows < 0 || !keys || !out_perm || !out_count || !ws_) {
        hs_set_error("hs_distinct: bad arguments");
        return HS_E_ARG;
    }
    int rc = ob_refuse_keys("hs_distinct", keys, n_keys, "columns");
    if (rc != HS_OK) return rc;
    *out_count = 0;
    if (nrows == 0) return HS_OK;
    if ((rc = ob_refuse_kinds("hs_distinct", keys, n_keys, "column", "compared")) != HS_OK) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const int32_t ascending[HS_MAX_COLS] = {0};
    ObSorted S;
    int64_t sorted_rows = 0;
    rc = ob_sort(stream, keys, ascending, n_keys, nrows, nrows_dev, -1, &sorted_rows, ws_, "hs_distinct", S);
    if (rc != HS_OK || S.count == 0) return rc;
    DhArgs D{ob_run(S, n_keys)};  // keep, mark: null
    // HIPSPARK_DISTINCT_GATHER=1 keeps the general path, so that tools/bench_distinct.py can time one against the other
    if (const char* gather = std::getenv("HIPSPARK_DISTINCT_GATHER"); gather && gather[0] == '1') D.words = nullptr;
    uint8_t* extra = (uint8_t*)ws_ + S.ws_bytes;  // behind what the sort laid out (hs_distinct_ws_bytes: at most hs_order_by_ws_bytes)
    D.keep = extra;
    int64_t* count_dev = (int64_t*)(extra + rx_align((size_t)nrows));
    void* scan_ws = (uint8_t*)count_dev + 256;
    const int64_t tiles = (D.n + OB_TILE - 1) / OB_TILE;
    hipLaunchKernelGGL(k_distinct_heads, dim3((unsigned)tiles), dim3(OB_THREADS), 0, stream, D);
    RX_CHECK_LAUNCH("hs_distinct (heads)");
    if ((rc = hs_compact(stream, D.keep, D.n, out_perm, count_dev, scan_ws)) != HS_OK) return rc;
    int64_t kept = 0;
    if (hipMemcpyAsync(&kept, count_dev, 8, hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess || kept < 1 || kept > D.n) {
        hs_set_error("hs_distinct: the compaction kept %lld rows of %lld", (long long)kept, (long long)D.n);
        return HS_E_LAUNCH;
    }
    *out_count = kept;
    return HS_OK;
}

// =====================================================================================================
// First-occurrence marks (include/hipspark.h hs_mark_first; the reference has no COUNT(DISTINCT)).
//
// marks[r] = 1 iff r is a considered row and no considered row before it has the same key words - hs_distinct's equality,
// hs_distinct's heads, written as an INTEGER column the partial aggregate SUMs: COUNT(DISTINCT e) GROUP BY k is the SUM of
// the marks over the keys (k, e).  Two ways to the same function of the rows:
//  * sort path: ob_sort over the considered rows (their list, or all), then k_distinct_heads into the zeroed marks.
//  * dense path, a key of ONE word whose varying bits V = AND ^ OR are few: the V bits of a word, squeezed together, index
//    a table first_row[1 << popcount(V)] of row numbers; k_mf_claim takes the minimum per slot (integer atomicMin: the
//    minimum does not depend on the order the atomics land in), k_mf_mark compares.  Rows are read once per kernel, marks
//    are written in input order, nothing is moved.
// =====================================================================================================
constexpr int MF_DENSE_BITS = 24;  // the table: 64 MB at most (profiles/r14_count_distinct.txt)
constexpr int MF_MAX_RUNS = 8;     // contiguous runs of V

struct MfArgs {
    const uint64_t* words;  // the key word of considered row i
    const int64_t* rows;    // its row number (null: i)
    int64_t n;
    uint32_t* first_row;    // [1 << popcount(V)]
    int32_t* marks;
    uint64_t run_mask[MF_MAX_RUNS];  // (1 << bits of the run) - 1
    int32_t run_shift[MF_MAX_RUNS];  // the run's lowest bit in the word
    int32_t run_at[MF_MAX_RUNS];     // ... and in the slot
    int32_t n_runs, pad;
};
static_assert(sizeof(MfArgs) % 8 == 0, "MfArgs");

__device__ __forceinline__ uint32_t mf_slot(const MfArgs& A, uint64_t word) {
    uint64_t slot = 0;
    for (int r = 0; r < A.n_runs; ++r) slot |= ((word >> A.run_shift[r]) & A.run_mask[r]) << A.run_at[r];
    return (uint32_t)slot;
}

__global__ void __launch_bounds__(OB_THREADS) k_mf_claim(const MfArgs A_kernarg) {
    HS_KERNARG(MfArgs, A);
    for (int64_t i = (int64_t)blockIdx.x * OB_THREADS + threadIdx.x; i < A.n; i += (int64_t)gridDim.x * OB_THREADS) {
        const uint32_t row = (uint32_t)(A.rows ? A.rows[i] : i);
        uint32_t* cell = A.first_row + mf_slot(A, A.words[i]);
        // a value read here is one some row wrote or the fill: never below the final minimum, so skipping is safe, and
        // with rows visited in rising order most values of a small domain skip the atomic
        if (*(volatile uint32_t*)cell > row) atomicMin(cell, row);
    }
}

__global__ void __launch_bounds__(OB_THREADS) k_mf_mark(const MfArgs A_kernarg) {
    HS_KERNARG(MfArgs, A);
    for (int64_t i = (int64_t)blockIdx.x * OB_THREADS + threadIdx.x; i < A.n; i += (int64_t)gridDim.x * OB_THREADS) {
        const int64_t row = A.rows ? A.rows[i] : i;
        A.marks[row] = A.first_row[mf_slot(A, A.words[i])] == (uint32_t)row ? 1 : 0;
    }
}

// the runs of `varying`, lowest first -> their number, or -1 when the dense path does not hold the word
static int mf_runs(uint64_t varying, MfArgs* A) {
    if (__builtin_popcountll(varying) > MF_DENSE_BITS) return -1;
    int n_runs = 0, at = 0;
    while (varying) {
        const int lo = __builtin_ctzll(varying);
        const int len = __builtin_ctzll(~(varying >> lo));  // at most MF_DENSE_BITS: the shifted word has a zero bit
        if (n_runs == MF_MAX_RUNS) return -1;
        if (A) {
            A->run_mask[n_runs] = (1ull << len) - 1ull;
            A->run_shift[n_runs] = lo;
            A->run_at[n_runs] = at;
        }
        ++n_runs;
        at += len;
        varying &= ~(((1ull << len) - 1ull) << lo);
    }
    return n_runs;
}
static bool mf_dense_fits(int32_t n_words, uint64_t varying) { return n_words == 1 && mf_runs(varying, nullptr) >= 0; }

extern "C" size_t hs_mark_first_ws_bytes(int64_t nrows, int32_t n_keys, int32_t max_key_words) {
    if (nrows < 0) return 0;
    // the sort's workspace, then the dense path's table at its largest
    return hs_order_by_ws_bytes(nrows, n_keys, max_key_words) + rx_align((size_t)4 << MF_DENSE_BITS);
}

extern "C" int hs_mark_first(void* stream_, const hs_col* keys, int32_t n_keys, int64_t nrows, const int64_t* sel,
                             int64_t n_sel, int32_t mode, int32_t* marks, void* ws_, uint32_t* flags) {
    (void)flags;
    if (n_keys <= 0 || nrows < 0 || !keys || !marks || !ws_ || mode < 0 || mode > 2 || (sel && (n_sel < 0 || n_sel > nrows))) {
        hs_set_error("hs_mark_first: bad arguments");
        return HS_E_ARG;
    }
    int rc = ob_refuse_keys("hs_mark_first", keys, n_keys, "columns");
    if (rc != HS_OK) return rc;
    if (nrows == 0) return HS_OK;
    if ((rc = ob_refuse_kinds("hs_mark_first", keys, n_keys, "column", "compared")) != HS_OK) return rc;
    const bool rows_fit = nrows < 0xffffffffll;  // a row number and the table's fill must differ
    if (mode == 2 && !rows_fit) {
        hs_set_error("hs_mark_first: the dense path holds row numbers below 2^32 - 1, not %lld rows", (long long)nrows);
        return HS_E_LIMIT;
    }
    hipStream_t stream = (hipStream_t)stream_;
    if (sel && hipMemsetAsync(marks, 0, (size_t)nrows * 4, stream) != hipSuccess) {  // without a list every row is written
        hs_set_error("hs_mark_first: clearing the marks failed");
        return HS_E_LAUNCH;
    }
    if (sel && n_sel == 0) return HS_OK;
    const int32_t ascending[HS_MAX_COLS] = {0};
    ObSorted S;
    int64_t considered = 0;
    const int dense = mode == 2 ? OB_DENSE_ONLY : (mode == 0 && rows_fit) ? OB_DENSE_IF_FITS : OB_SORT;
    rc = ob_sort(stream, keys, ascending, n_keys, nrows, nullptr, -1, &considered, ws_, "hs_mark_first", S, sel, sel ? n_sel : 0,
                 dense);
    if (rc != HS_OK || S.count == 0) return rc;
    if (S.unsorted) {
        MfArgs M;
        std::memset(&M, 0, sizeof(M));
        M.n_runs = S.n_words == 1 ? mf_runs(S.varying, &M) : -1;
        if (M.n_runs < 0) {  // mode 2 only: in mode 0 the sort went on unless the key fits
            hs_set_error("hs_mark_first: the dense path takes a key of one word whose varying bits are at most %d in at most "
                         "%d runs (this key: %d words, varying bits %016llx)", MF_DENSE_BITS, MF_MAX_RUNS, S.n_words,
                         (unsigned long long)S.varying);
            return HS_E_LIMIT;
        }
        M.words = S.words;
        M.rows = sel ? S.rows : nullptr;  // without a list the sort's row list is 0, 1, 2 ...: not read
        M.n = S.n;
        M.first_row = (uint32_t*)((uint8_t*)ws_ + S.ws_bytes);
        M.marks = marks;
        const size_t table_bytes = (size_t)4 << __builtin_popcountll(S.varying);
        if (hipMemsetAsync(M.first_row, 0xff, table_bytes, stream) != hipSuccess) {
            hs_set_error("hs_mark_first: filling the table failed");
            return HS_E_LAUNCH;
        }
        hipLaunchKernelGGL(k_mf_claim, dim3(ob_grid(M.n)), dim3(OB_THREADS), 0, stream, M);
        hipLaunchKernelGGL(k_mf_mark, dim3(ob_grid(M.n)), dim3(OB_THREADS), 0, stream, M);
        RX_CHECK_LAUNCH("hs_mark_first (dense)");
        return HS_OK;
    }
    DhArgs D{ob_run(S, n_keys)};
    if (!S.n_words) D.perm = sel;  // a key without a byte: every considered row is equal, the first of them the head
    D.mark = marks;
    const int64_t tiles = (D.n + OB_TILE - 1) / OB_TILE;
    hipLaunchKernelGGL(k_distinct_heads, dim3((unsigned)tiles), dim3(OB_THREADS), 0, stream, D);
    RX_CHECK_LAUNCH("hs_mark_first (heads)");
    return HS_OK;
}

// =====================================================================================================
// Window functions over result rows (include/hipspark.h hs_window, hs_window_agg, hs_window_nav, hs_window_frames; the
// reference has no window functions).  What the four entries share stands here; ranking, aggregates, navigation and the
// sliding frames follow.
//
// ob_sort orders the rows by (partition columns, order keys): a partition is a run of sorted positions, peers are
// neighbours, and the sort being stable the rows of a group of peers stand in input order.  k_win_heads writes two bits
// per SORTED position - the row differs from its left neighbour in any key byte (peer head) / in the first `part_bytes`
// bytes of the key (partition head) - with k_distinct_heads' neighbour shuffle.  Everything else is a SEGMENTED SCAN over the positions: a
// summary (p, q, x) of a range of positions - p / q the last partition / peer head in it (-1: none), x a third field
// that restarts at every partition head - joins with the summary of the positions behind it as
//     (p, q, x) (+) (p', q', x') = (max(p, p'), max(q, q'), p' >= 0 ? x' : x op x')
// associative, NOT commutative: every level joins with the earlier positions on the LEFT.  Two summaries: WinS, x = d,
// the peer heads since the partition head (op: +, identity 0), and WinA, x = a, a 64-bit fold of an argument (op chosen
// at run time).  Each has an "ops" type with none() (the identity), join(earlier, later) and shfl_up(v, d); the rest is
// written once over it, on OB_TILE-row tiles, a lane holding WIN_PER = 8 consecutive positions (one 8-byte load of head
// bytes, WinLane):
//   win_fold_lane    a lane's 8 positions joined left to right;
//   win_block_excl   the exclusive scan of one summary per thread over the workgroup: the __shfl_up ladder inside a wave,
//                    one LDS hop across the four waves, joined in order;
//   k_win_tiles      one workgroup, rounds of OB_TILE tile summaries, the carry of the rounds before on the left: every
//                    tile's summary becomes the tile's carry - the join of all tiles before it - in place;
//   win_rescan_lane  a tile scanned again behind its carry: put(k, run) gets the inclusive summary at each of the lane's
//                    positions that is a row.  The kernels that scatter to rows hand what they need over through LDS
//                    - a lane writes its 8 positions at win_put_at, consecutive lanes read consecutive positions at
//                    win_get_at, one pad word per lane segment (k_scan_down's layout) - so that the row list is read
//                    coalesced.
// A tile without a head has the summary none() and passes its carry on as it is.  Positions are int32: rows < 2^31.
// =====================================================================================================
constexpr int WIN_PER = OB_TILE / OB_THREADS;  // consecutive sorted positions of a lane in the scan passes
static_assert(WIN_PER == 8, "a lane's head bytes are one 8-byte load");

struct WinHeads : ObRun {
    int64_t part_bytes;     // the partition columns' bytes: the first part_bytes bytes of a row's key
    uint8_t* heads;         // by sorted position: bit 0 peer head, bit 1 partition head
};
static_assert(sizeof(WinHeads) == sizeof(ObRun) + 16, "WinHeads");
// a kernel argument is ObRun's members, then the struct's own directly behind them
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winvalid-offsetof"  // a struct with a base is no standard-layout type; clang lays it out as C would
static_assert(offsetof(DhArgs, keep) == sizeof(ObRun) && offsetof(WinHeads, part_bytes) == sizeof(ObRun), "behind ObRun");
#pragma clang diagnostic pop

// the bytes of word w that belong to the partition prefix (byte 0 of the key = most significant byte of word 0)
__device__ __forceinline__ uint64_t win_part_mask(int64_t part_bytes, int32_t w) {
    const int64_t in = part_bytes - 8 * (int64_t)w;
    return in >= 8 ? ~0ull : in <= 0 ? 0ull : ~0ull << (8 * (8 - in));
}

__global__ void __launch_bounds__(OB_THREADS) k_win_heads(const WinHeads A_kernarg) {
    HS_KERNARG(WinHeads, A);
    const int lane = threadIdx.x & (HS_WAVE - 1), wave = threadIdx.x / HS_WAVE;
    const int64_t first = (int64_t)blockIdx.x * OB_TILE + (int64_t)wave * (OB_STEPS * HS_WAVE) + lane;
    for (int j = 0; j < OB_STEPS; ++j) {
        const int64_t i = first + j * HS_WAVE;
        if (i - lane >= A.n) break;                   // the whole wave step lies past the rows
        const bool live = i < A.n;
        const int64_t pos = live ? i : A.n - 1;       // lanes past the end repeat the last row: every read stays inside
        bool peer = false, part = false;
        if (A.words) {  // coalesced: the sort's own words
            const unsigned long long mine = A.words[pos];
            unsigned long long left = __shfl_up(mine, 1, HS_WAVE);
            if (lane == 0) left = i > 0 ? A.words[i - 1] : mine;
            const unsigned long long diff = mine ^ left;
            peer = diff != 0;
            part = (diff & win_part_mask(A.part_bytes, 0)) != 0;
        } else if (A.n_words > 0) {
            const int64_t row = A.perm[pos];
            // lane 0's left neighbour sits in no lane of this step: sorted position i - 1, loaded explicitly
            const int64_t before = (lane == 0 && i > 0) ? A.perm[i - 1] : row;
            for (int32_t w = 0; w < A.n_words; ++w) {  // most significant first: a lane's first differing word decides both bits
                const unsigned long long mine = ob_word(A.K, A.n_keys, w, row);
                unsigned long long left = __shfl_up(mine, 1, HS_WAVE);
                if (lane == 0) left = ob_word(A.K, A.n_keys, w, before);
                const unsigned long long diff = mine ^ left;
                peer |= diff != 0;
                part |= (diff & win_part_mask(A.part_bytes, w)) != 0;
                if (__ballot(!peer) == 0) break;      // every lane of the step has found its difference
            }
        }
        if (i == 0) peer = part = true;
        if (live) A.heads[i] = (uint8_t)((peer ? 1 : 0) | (part ? 2 : 0));
    }
}

struct WinS {
    int32_t p, q, d;  // last partition head, last peer head (-1: none in the range), peer heads since the partition head
};
// a WinS as the tile records hold it: 16 bytes, one vector load or store (in LDS a WinS stays 12 bytes)
struct alignas(16) WinRec {
    int32_t p, q, d, zero;
    WinRec() = default;
    __device__ WinRec(const WinS s) : p(s.p), q(s.q), d(s.d), zero(0) {}
    __device__ operator WinS() const { return WinS{p, q, d}; }
};
static_assert(sizeof(WinRec) == 16, "WinRec");
struct WinSOps {
    using S = WinS;
    using Rec = WinRec;
    __device__ __forceinline__ WinS none() const { return WinS{-1, -1, 0}; }
    __device__ __forceinline__ WinS join(const WinS a, const WinS b) const {  // a: the EARLIER positions
        return WinS{a.p > b.p ? a.p : b.p, a.q > b.q ? a.q : b.q, b.p >= 0 ? b.d : a.d + b.d};
    }
    __device__ __forceinline__ WinS shfl_up(const WinS v, int d) const {
        return WinS{__shfl_up(v.p, d, HS_WAVE), __shfl_up(v.q, d, HS_WAVE), __shfl_up(v.d, d, HS_WAVE)};
    }
    // the third field of ONE position: it counts itself where it is a peer head (the cell is not looked at)
    __device__ __forceinline__ int32_t third(uint32_t head, uint64_t) const { return (int32_t)(head & 1u); }
};

enum { WA_NONE = 0, WA_ADD_I = 1, WA_ADD_F = 2, WA_MIN = 3, WA_MAX = 4 };

struct WinA {
    int32_t p, q;  // as in WinS
    uint64_t a;    // the fold since the last partition head
};
static_assert(sizeof(WinA) == 16, "WinA");

__device__ __forceinline__ uint64_t wa_identity(int op) { return op == WA_MIN ? ~0ull : 0ull; }
__device__ __forceinline__ uint64_t wa_op(int op, uint64_t a, uint64_t b) {  // a: the EARLIER positions
    switch (op) {
        case WA_ADD_I: return a + b;
        case WA_ADD_F: return hs_d2u(hs_u2d(a) + hs_u2d(b));
        case WA_MIN: return a < b ? a : b;
        case WA_MAX: return a > b ? a : b;
        default: return 0;
    }
}
struct WinAOps {
    using S = WinA;
    using Rec = WinA;
    int32_t op;
    __device__ __forceinline__ WinA none() const { return WinA{-1, -1, wa_identity(op)}; }
    __device__ __forceinline__ WinA join(const WinA a, const WinA b) const {  // a: the EARLIER positions
        return WinA{a.p > b.p ? a.p : b.p, a.q > b.q ? a.q : b.q, b.p >= 0 ? b.a : wa_op(op, a.a, b.a)};
    }
    __device__ __forceinline__ WinA shfl_up(const WinA v, int d) const {
        return WinA{__shfl_up(v.p, d, HS_WAVE), __shfl_up(v.q, d, HS_WAVE),
                    (uint64_t)__shfl_up((unsigned long long)v.a, d, HS_WAVE)};  // two 32-bit shuffles
    }
    __device__ __forceinline__ uint64_t third(uint32_t, uint64_t x) const { return x; }  // the position's lifted cell
};

// the summary of ONE position j with head bits `head`
template <typename S, typename T>
__device__ __forceinline__ S win_of(uint32_t head, int32_t j, T third) {
    return S{(head & 2u) ? j : -1, (head & 1u) ? j : -1, third};
}

// A lane's WIN_PER consecutive positions of its workgroup's tile and their head bytes
struct WinLane {
    int64_t j0, n;
    uint64_t bytes;
    // head bits of position j0 + k, k-th byte of the lane's load; nothing past the rows
    __device__ __forceinline__ uint32_t head(int k) const { return j0 + k < n ? (uint32_t)(bytes >> (8 * k)) & 3u : 0u; }
};
__device__ __forceinline__ WinLane win_lane(const uint8_t* heads, int64_t n) {
    const int64_t j0 = (int64_t)blockIdx.x * OB_TILE + (int64_t)threadIdx.x * WIN_PER;
    return WinLane{j0, n, *(const uint64_t*)(heads + j0)};  // the buffer holds whole tiles
}
struct WinNoCells {  // WinS looks at no cell
    __device__ __forceinline__ uint64_t operator()(int) const { return 0; }
};
// the lane's positions joined left to right; x(k): the lifted cell of position j0 + k
template <typename O, typename X>
__device__ __forceinline__ typename O::S win_fold_lane(const O o, const WinLane& L, X x) {
    typename O::S acc = o.none();
#pragma unroll
    for (int k = 0; k < WIN_PER; ++k)
        acc = o.join(acc, win_of<typename O::S>(L.head(k), (int32_t)(L.j0 + k), o.third(L.head(k), x(k))));
    return acc;
}

// exclusive scan of one summary per thread over the workgroup, in thread order; `total` = the join of all (every thread).
// Wave shuffles, then one LDS hop across the four waves.  The caller puts a barrier before s_wave is used again.
template <typename O>
__device__ __forceinline__ typename O::S win_block_excl(const O o, const typename O::S v, typename O::S* s_wave,
                                                        typename O::S& total) {
    typedef typename O::S S;
    const int lane = threadIdx.x & (HS_WAVE - 1), w = threadIdx.x / HS_WAVE;
    S incl = v;
#pragma unroll
    for (int d = 1; d < HS_WAVE; d <<= 1) {
        const S t = o.shfl_up(incl, d);
        if (lane >= d) incl = o.join(t, incl);
    }
    if (lane == HS_WAVE - 1) s_wave[w] = incl;
    S excl = o.shfl_up(incl, 1);
    if (lane == 0) excl = o.none();
    __syncthreads();
    S base = o.none();
    total = base;
#pragma unroll
    for (int k = 0; k < OB_WAVES; ++k) {
        if (k == w) base = total;
        total = o.join(total, s_wave[k]);
    }
    return o.join(base, excl);
}

// one workgroup: sums[t] = the join of the summaries of tiles 0 .. t - 1 (tile t's carry), in place
template <typename O>
__global__ void __launch_bounds__(OB_THREADS) k_win_tiles(typename O::Rec* sums, int64_t ntiles, const O o) {
    typedef typename O::S S;
    __shared__ S s_wave[OB_WAVES];
    S carry = o.none();  // the rounds before this one: the same in every thread
    for (int64_t t0 = 0; t0 < ntiles; t0 += OB_TILE) {
        const int64_t mine = t0 + (int64_t)threadIdx.x * WIN_PER;
        S v[WIN_PER], acc = o.none();
#pragma unroll
        for (int k = 0; k < WIN_PER; ++k) {
            v[k] = o.none();
            if (mine + k < ntiles) v[k] = sums[mine + k];
            acc = o.join(acc, v[k]);
        }
        S total;
        S run = o.join(carry, win_block_excl(o, acc, s_wave, total));
#pragma unroll
        for (int k = 0; k < WIN_PER; ++k) {
            if (mine + k < ntiles) sums[mine + k] = run;
            run = o.join(run, v[k]);
        }
        carry = o.join(carry, total);
        __syncthreads();
    }
}

// a tile scanned again behind its carry: put(k, run), run the join of everything through position j0 + k, for the lane's
// positions that are rows (the step's join stays inside the test: joined ahead of it, eight summaries are live at once)
template <typename O, typename X, typename Put>
__device__ __forceinline__ void win_rescan_lane(const O o, const WinLane& L, X x, const typename O::S carry,
                                                typename O::S* s_wave, Put put) {
    typename O::S total;
    typename O::S run = o.join(carry, win_block_excl(o, win_fold_lane(o, L, x), s_wave, total));
#pragma unroll
    for (int k = 0; k < WIN_PER; ++k)
        if (L.j0 + k < L.n) {
            run = o.join(run, win_of<typename O::S>(L.head(k), (int32_t)(L.j0 + k), o.third(L.head(k), x(k))));
            put(k, run);
        }
}
// ... of (p, q, d), what the kernels that scatter to rows start with
template <typename Put>
__device__ __forceinline__ void win_rescan(const uint8_t* heads, const WinS carry, int64_t n, WinS* s_wave, Put put) {
    win_rescan_lane(WinSOps{}, win_lane(heads, n), WinNoCells{}, carry, s_wave, put);
}
// the LDS hand-over: where lane `tid` puts its k-th position, where element e = k * OB_THREADS + tid of the tile is read
__device__ __forceinline__ int win_put_at(int tid, int k) { return tid * (WIN_PER + 1) + k; }
__device__ __forceinline__ int win_get_at(int e) { return e + e / WIN_PER; }

// what every kernel behind the front half starts from
struct WinTile {
    const uint8_t* heads;  // by sorted position, whole tiles
    const int64_t* perm;   // the sorted rows (null: position = row)
    const WinRec* carry;   // per tile: (p, q, d) of the tiles before (k_win_tiles)
    int64_t n;
};

// -----------------------------------------------------------------------------------------------------
// Ranking (hs_window).  Per position j the answers are
//     row_number = j - P + 1      P: the last partition head at or before j
//     rank       = Q - P + 1      Q: the last peer head at or before j
//     dense_rank = D              D: the peer heads in [P, j]
// P and Q are max-scans of head positions, D the segmented sum: WinS.  k_win_reduce folds a tile into one summary,
// k_win_tiles turns the summaries into carries, k_win_emit scans the tile again and scatters ONE function's values to the
// rows: out[perm[j]] - a launch per requested function, the scan being cheap next to the scatter.
// -----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(OB_THREADS) k_win_reduce(const uint8_t* heads, int64_t n, WinRec* sums) {
    __shared__ WinS s_wave[OB_WAVES];
    const WinSOps o{};
    WinS total;
    win_block_excl(o, win_fold_lane(o, win_lane(heads, n), WinNoCells{}), s_wave, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

struct WinEmit : WinTile {
    int32_t* out;       // one function per launch: three scattered columns at once fall out of the last-level cache
    int32_t func, pad;  // that one column's partial lines still merge in (profiles/r15_window.txt)
};
static_assert(sizeof(WinEmit) % 8 == 0, "WinEmit");

__global__ void __launch_bounds__(OB_THREADS) k_win_emit(const WinEmit A_kernarg) {
    HS_KERNARG(WinEmit, A);
    __shared__ WinS s_wave[OB_WAVES];
    __shared__ int32_t s_p[OB_TILE + OB_THREADS], s_q[OB_TILE + OB_THREADS], s_d[OB_TILE + OB_THREADS];
    const int tid = threadIdx.x;
    const int64_t tile0 = (int64_t)blockIdx.x * OB_TILE;
    win_rescan(A.heads, A.carry[blockIdx.x], A.n, s_wave, [&](int k, const WinS run) {
        s_p[win_put_at(tid, k)] = run.p;
        s_q[win_put_at(tid, k)] = run.q;
        s_d[win_put_at(tid, k)] = run.d;
    });
    __syncthreads();
#pragma unroll
    for (int k = 0; k < WIN_PER; ++k) {
        const int e = k * OB_THREADS + tid;
        const int64_t j = tile0 + e;
        if (j >= A.n) break;
        const int64_t row = A.perm ? A.perm[j] : j;
        const int32_t p = s_p[win_get_at(e)], q = s_q[win_get_at(e)], d = s_d[win_get_at(e)];
        A.out[row] = A.func == HS_WIN_ROW_NUMBER ? (int32_t)j - p + 1 : A.func == HS_WIN_RANK ? q - p + 1 : d;
    }
}

// -----------------------------------------------------------------------------------------------------
// Aggregates (hs_window_agg).  COUNT / SUM / AVG / MIN / MAX: per sorted position j the value is the fold
// of the argument over [P(j), E(j)], E the frame's end: j itself (ROWS), the last peer of j (RANGE), the partition's last
// row (PARTITION).  The fold is WinA's third field - the restart is a select, so a NaN or an infinity never leaves its
// partition - with a 64-bit accumulator: an i64 sum, an f64 sum, or for MIN / MAX the sort's order-preserving word of the
// cell (ob_f32_word: -0.0 = 0.0, NaN after +inf).  Earlier positions stay on the LEFT at every level, so the association
// of an f64 sum is fixed by (rows, tile geometry): the same bits from run to run, not those of the left-to-right fold.
// Per item:
//   k_wagg_reduce  gathers the argument through the row list (coalesced over positions, across to the lanes' 8
//                  consecutive positions through LDS), leaves the cells in SORTED order for the next pass and folds the
//                  tile into one summary;
//   k_win_tiles    over WinA: every tile's carry;
//   k_wagg_scan    scans the tile again behind both carries and, at every frame end, stores the running value and the
//                  frame's row count into two tables indexed by the frame's START position (j, Q or P): one vector
//                  store per frame, no atomics;
//   k_wagg_emit    every position reads the tables at its own j / Q / P - all rows of a frame the same cell - finishes
//                  the value (AVG divides, SUM / AVG round to the cell type and raise the overflow flags) and scatters
//                  out[perm[j]], one launch per item like k_win_emit.
// COUNT has no argument: it skips the first two kernels; COUNT under ROWS is ROW_NUMBER and takes k_win_emit.
// -----------------------------------------------------------------------------------------------------
// a stored cell as an accumulator
__device__ __forceinline__ uint64_t wa_lift(int op, int is_float, uint32_t v) {
    switch (op) {
        case WA_ADD_I: return (uint64_t)(int64_t)(int32_t)v;
        case WA_ADD_F: return hs_d2u((double)__uint_as_float(v));
        case WA_MIN:
        case WA_MAX: return is_float ? ob_f32_word(v) : v ^ 0x80000000u;
        default: return 0;
    }
}
// x[k] = the lifted cell(k) of the lane's k-th position; the identity past the rows, where no cell is looked at
template <typename Cell>
__device__ __forceinline__ void wa_lift_lane(int op, int is_float, const WinLane& L, Cell cell, uint64_t (&x)[WIN_PER]) {
#pragma unroll
    for (int k = 0; k < WIN_PER; ++k) x[k] = L.j0 + k < L.n ? wa_lift(op, is_float, cell(k)) : wa_identity(op);
}

struct WaggArgs : WinTile {
    const uint32_t* values;  // the argument's cells, input order (not read when op == WA_NONE)
    uint32_t* sorted;        // the cells by sorted position, whole tiles
    WinA* tiles;             // per tile: k_wagg_reduce's summary, then k_win_tiles' carry
    uint64_t* tab_a;         // by the START position of a frame: its fold ...
    int32_t* tab_c;          // ... and its rows
    uint32_t* out;           // one item per launch: input order
    uint32_t* flags;         // may be null
    int32_t op, is_float, frame, func;
};
static_assert(sizeof(WaggArgs) % 8 == 0, "WaggArgs");

__global__ void __launch_bounds__(OB_THREADS) k_wagg_reduce(const WaggArgs A_kernarg) {
    HS_KERNARG(WaggArgs, A);
    __shared__ WinA s_wave[OB_WAVES];
    __shared__ uint32_t s_v[OB_TILE + OB_THREADS];
    const int tid = threadIdx.x;
    const WinAOps o{A.op};
    const int64_t tile0 = (int64_t)blockIdx.x * OB_TILE;
#pragma unroll
    for (int k = 0; k < WIN_PER; ++k) {
        const int e = k * OB_THREADS + tid;
        const int64_t j = tile0 + e;
        uint32_t v = 0;
        if (j < A.n) {
            v = A.values[A.perm ? A.perm[j] : j];
            A.sorted[j] = v;
        }
        s_v[win_get_at(e)] = v;
    }
    __syncthreads();
    const WinLane L = win_lane(A.heads, A.n);
    uint64_t x[WIN_PER];
    wa_lift_lane(o.op, A.is_float, L, [&](int k) { return s_v[win_put_at(tid, k)]; }, x);
    WinA total;
    win_block_excl(o, win_fold_lane(o, L, [&](int k) { return x[k]; }), s_wave, total);
    if (tid == 0) A.tiles[blockIdx.x] = total;
}

__global__ void __launch_bounds__(OB_THREADS) k_wagg_scan(const WaggArgs A_kernarg) {
    HS_KERNARG(WaggArgs, A);
    __shared__ WinA s_wave[OB_WAVES];
    const WinAOps o{A.op};
    const int frame = A.frame;
    const WinLane L = win_lane(A.heads, A.n);
    // the head byte behind the lane's eight: written where it is a row (the byte after the last tile is never read)
    const uint32_t next = L.j0 + WIN_PER < A.n ? A.heads[L.j0 + WIN_PER] : 0u;
    uint32_t cell[WIN_PER] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (o.op != WA_NONE) {  // `sorted` holds whole tiles: cells past the rows are read and not used
        const uint4 lo = *(const uint4*)(A.sorted + L.j0), hi = *(const uint4*)(A.sorted + L.j0 + 4);
        cell[0] = lo.x, cell[1] = lo.y, cell[2] = lo.z, cell[3] = lo.w;
        cell[4] = hi.x, cell[5] = hi.y, cell[6] = hi.z, cell[7] = hi.w;
    }
    uint64_t x[WIN_PER];
    wa_lift_lane(o.op, A.is_float, L, [&](int k) { return cell[k]; }, x);
    const WinS c = A.carry[blockIdx.x];
    const uint64_t ca = o.op != WA_NONE ? A.tiles[blockIdx.x].a : 0ull;
    const uint32_t end_bit = frame == HS_WIN_FRAME_RANGE ? 1u : 2u;
    win_rescan_lane(o, L, [&](int k) { return x[k]; }, WinA{c.p, c.q, ca}, s_wave, [&](int k, const WinA run) {
        const int64_t j = L.j0 + k;
        const uint32_t after = k + 1 < WIN_PER ? (uint32_t)(L.bytes >> (8 * (k + 1))) : next;
        // a frame ends where the next position starts another run of peers / another partition, and at the last row
        if (frame == HS_WIN_FRAME_ROWS || j + 1 >= A.n || (after & end_bit)) {
            const int32_t start = frame == HS_WIN_FRAME_ROWS ? (int32_t)j : frame == HS_WIN_FRAME_RANGE ? run.q : run.p;
            A.tab_a[start] = run.a;
            A.tab_c[start] = (int32_t)j - run.p + 1;
        }
    });
}

__device__ __forceinline__ uint32_t wa_f32(double d, uint32_t& err) {
    const float f = (float)d;  // RNE
    if (isinf(f) && !isinf(d)) err |= HS_FLAG_FLT_OVERFLOW;
    return __float_as_uint(f);
}
// the cell an item stores for a frame's fold `a` over `count` rows
__device__ __forceinline__ uint32_t wa_finish(int func, int is_float, uint64_t a, int32_t count, uint32_t& err) {
    switch (func) {
        case HS_WIN_COUNT: return (uint32_t)count;
        case HS_WIN_SUM:
            if (is_float) return wa_f32(hs_u2d(a), err);
            if ((int64_t)a != (int64_t)(int32_t)a) err |= HS_FLAG_INT_OVERFLOW;
            return (uint32_t)a;
        case HS_WIN_AVG: return wa_f32((is_float ? hs_u2d(a) : (double)(int64_t)a) / (double)count, err);
        default: {  // MIN / MAX: the word back to the cell
            const uint32_t w = (uint32_t)a;
            if (!is_float) return w ^ 0x80000000u;
            return (w & 0x80000000u) ? (w & 0x7fffffffu) : ~w;
        }
    }
}

__global__ void __launch_bounds__(OB_THREADS) k_wagg_emit(const WaggArgs A_kernarg) {
    HS_KERNARG(WaggArgs, A);
    __shared__ WinS s_wave[OB_WAVES];
    __shared__ int32_t s_at[OB_TILE + OB_THREADS];  // the table cell of every position
    const int tid = threadIdx.x, frame = A.frame;
    const int64_t tile0 = (int64_t)blockIdx.x * OB_TILE, j0 = tile0 + (int64_t)tid * WIN_PER;
    win_rescan(A.heads, A.carry[blockIdx.x], A.n, s_wave, [&](int k, const WinS run) {
        s_at[win_put_at(tid, k)] = frame == HS_WIN_FRAME_ROWS ? (int32_t)(j0 + k) : frame == HS_WIN_FRAME_RANGE ? run.q : run.p;
    });
    __syncthreads();
    uint32_t err = 0;
#pragma unroll
    for (int k = 0; k < WIN_PER; ++k) {
        const int e = k * OB_THREADS + tid;
        const int64_t j = tile0 + e;
        if (j < A.n) {
            const int64_t row = A.perm ? A.perm[j] : j;
            const int32_t at = s_at[win_get_at(e)];
            A.out[row] = wa_finish(A.func, A.is_float, A.tab_a[at], A.tab_c[at], err);
        }
    }
    if (err && A.flags) atomicOr(A.flags, err);
}

// -----------------------------------------------------------------------------------------------------
// Navigation (hs_window_nav).  LAG / LEAD / FIRST_VALUE / LAST_VALUE copy the argument's cell of ANOTHER
// sorted position s of the row's partition, NTILE numbers buckets from (row number, partition rows).  Per sorted position
// j, P / Q the partition / peer head at or before j and E the frame's end:
//     LAG(k)       s = j - k, the default when s < P         LEAD(k)  s = j + k, the default when s > E(partition)
//     FIRST_VALUE  s = P                                     LAST_VALUE  s = j (ROWS) | E(range) | E(partition)
//     NTILE(n)     r = j - P + 1 of N = E(partition) - P + 1 rows
// E comes from k_wagg_scan run without an argument (WA_NONE): it leaves tab_c[start] = E - P + 1 at start = P (PARTITION) or
// Q (RANGE) - one pass per frame the call needs, not per item.  Per distinct argument k_wnav_gather leaves the cells in
// sorted order (4 or 8 bytes; without keys position = row and the argument is read as it stands), per item k_wnav_emit
// rescans (p, q), reads cell s and scatters out[perm[j]].  Cells are copied as bits.
// -----------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(OB_THREADS) k_wnav_gather(const int64_t* perm, const T* values, T* sorted, int64_t n) {
    const int64_t tile0 = (int64_t)blockIdx.x * OB_TILE;
    int64_t row[WIN_PER];
#pragma unroll
    for (int k = 0; k < WIN_PER; ++k) {  // consecutive lanes on consecutive positions; nothing past the rows
        const int64_t j = tile0 + k * OB_THREADS + threadIdx.x;
        row[k] = j < n ? perm[j] : -1;
    }
#pragma unroll
    for (int k = 0; k < WIN_PER; ++k)
        if (row[k] >= 0) sorted[tile0 + k * OB_THREADS + threadIdx.x] = values[row[k]];
}

struct WnavArgs : WinTile {
    const void* cells;     // the argument by sorted position (not read by NTILE)
    const int32_t* tab_c;  // E - P + 1 by the frame's start (LEAD, NTILE: PARTITION; LAST_VALUE: its frame's; else not read)
    void* out;             // one item per launch: input order
    uint64_t dflt;         // LAG / LEAD: the default's bits
    int64_t k;             // LAG / LEAD: the offset; NTILE: the buckets; FIRST_VALUE / LAST_VALUE under HS_WIN_FRAME_BETWEEN:
    int32_t func, frame;   // the frame's n PRECEDING / m FOLLOWING (4.4i)
};
static_assert(sizeof(WnavArgs) % 8 == 0, "WnavArgs");

// NTILE: the bucket of row r (1-based) of N rows in n buckets, the first N mod n of them one row larger
__device__ __forceinline__ uint32_t wnav_ntile(uint32_t r, uint32_t N, uint32_t n) {
    const uint32_t s = N / n, m = N - s * n, big = m * (s + 1);  // big <= N: no overflow
    if (r <= big) return (r - 1) / (s + 1) + 1;
    return m + (r - 1 - big) / (s ? s : 1u) + 1;                 // s == 0: big == N, never here
}

template <typename T>
__global__ void __launch_bounds__(OB_THREADS) k_wnav_emit(const WnavArgs A_kernarg) {
    HS_KERNARG(WnavArgs, A);
    __shared__ WinS s_wave[OB_WAVES];
    __shared__ int32_t s_p[OB_TILE + OB_THREADS], s_q[OB_TILE + OB_THREADS];
    const int tid = threadIdx.x, func = A.func, frame = A.frame;
    const int64_t tile0 = (int64_t)blockIdx.x * OB_TILE;
    win_rescan(A.heads, A.carry[blockIdx.x], A.n, s_wave, [&](int k, const WinS run) {
        s_p[win_put_at(tid, k)] = run.p;
        s_q[win_put_at(tid, k)] = run.q;
    });
    __syncthreads();
    const T* cells = (const T*)A.cells;
    T* out = (T*)A.out;
#pragma unroll
    for (int k = 0; k < WIN_PER; ++k) {
        const int e = k * OB_THREADS + tid;
        const int64_t j = tile0 + e;
        if (j >= A.n) break;
        const int64_t row = A.perm ? A.perm[j] : j;
        const int64_t p = s_p[win_get_at(e)], q = s_q[win_get_at(e)];  // 0 <= p <= q <= j: position 0 is a head
        if (func == HS_WIN_NTILE) {
            out[row] = (T)wnav_ntile((uint32_t)(j - p + 1), (uint32_t)A.tab_c[p], (uint32_t)A.k);
            continue;
        }
        int64_t s = j;  // 64 bits: k may be 2^31 - 1
        bool valid = true;
        if (func == HS_WIN_LAG) {
            s = j - A.k;
            valid = s >= p;
        } else if (func == HS_WIN_LEAD) {
            s = j + A.k;
            valid = s <= p + A.tab_c[p] - 1;
        } else if (func == HS_WIN_FIRST_VALUE) {
            s = frame == HS_WIN_FRAME_BETWEEN && j - A.k > p ? j - A.k : p;  // k PRECEDING, clamped to the partition's first row
        } else if (frame == HS_WIN_FRAME_BETWEEN) {  // LAST_VALUE, k FOLLOWING, clamped to the partition's last row
            const int64_t last = p + A.tab_c[p] - 1;
            s = j + A.k < last ? j + A.k : last;
        } else if (frame != HS_WIN_FRAME_ROWS) {  // LAST_VALUE: the frame's last row
            s = p + A.tab_c[frame == HS_WIN_FRAME_RANGE ? q : p] - 1;
        }
        out[row] = valid ? cells[s] : (T)A.dflt;  // a valid s lies in the row's partition: inside [0, n)
    }
}

// -----------------------------------------------------------------------------------------------------
// Sliding frames (hs_window_frames).  ROWS BETWEEN n PRECEDING AND m FOLLOWING: per sorted position j the
// frame is [lo, hi] = [max(P, j - n), min(L, j + m)], P / L the first / last position of j's partition.  Both ends move,
// so no fold from the partition head answers it, and the difference of two running folds is not taken: it would carry a
// NaN or an infinity out of its frame (inf - inf) and cancel.  Instead every partition is cut into BLOCKS of
// W = n + m + 1 positions counted from P - block heads where (j - P) mod W == 0 - and two folds restart at them:
//     pre[j] = the fold from j's block head through j          (WinA over the block-head bytes, left to right)
//     suf[j] = the fold from j through the end of j's block    (the same scan over the MIRRORED positions n - 1 - j,
//                                                               whose heads are the block ends)
// A frame is at most W long, so it starts at a block head, ends at a block end, or crosses exactly one block boundary:
//     lo, hi in different blocks: suf[lo] op pre[hi]     same block, lo its head: pre[hi]     else (hi its end): suf[lo]
// two table reads and one op per row whatever W is, and nothing outside the frame is ever folded in.  COUNT is
// hi - lo + 1.  L = P + rows - 1 from navigation's PARTITION end table.  W and the positions are 64-bit on the host; on
// the device W is capped at 2^31 (no partition is longer), which keeps the division at 32 bits.
// FLOAT sums: pre is joined with the earlier positions on the left at every level, suf with the LATER positions on the
// left (f64 addition commutes, so only the association differs); the association is fixed by (rows, n, m, tile
// geometry): the same bits from run to run, not those of the left-to-right fold of the frame.
// Per item with an argument:
//   k_wfr_heads    rescans (p, q, d) and writes both head byte rows (kept while the next item has the same W);
//   k_wnav_gather  the cells in sorted order (32-bit);
//   k_wfr_reduce   grid.y = direction: a tile's cells, coalesced and across to the lanes through LDS, folded to a summary;
//   k_win_tiles    over WinA, once per direction;
//   k_wfr_scan     grid.y = direction: the tile scanned again behind its carry, pre / suf stored per position;
//   k_wfr_emit     per position: P by rescan, L, lo, hi, the case above, wa_finish, out[perm[j]] - one launch per item.
// FIRST_VALUE / LAST_VALUE read the sorted cell at lo / hi in k_wnav_emit.  No atomics on values, no scratch.
// -----------------------------------------------------------------------------------------------------
struct WfrArgs : WinTile {
    const int32_t* part_rows;  // the partition's rows by its head position (navigation's PARTITION end table)
    const uint32_t* sorted;    // the argument's cells by sorted position: exactly n of them
    uint8_t* bheads[2];        // block heads by position / block ends by mirrored position, bit 1, whole tiles
    WinA* tiles[2];            // per tile and direction: k_wfr_reduce's summary, then k_win_tiles' carry
    uint64_t* tab[2];          // pre / suf by sorted position
    uint32_t* out;             // one item per launch: input order
    uint32_t* flags;           // may be null
    int64_t preceding, following;
    uint32_t width;            // min(W, 2^31)
    int32_t op, is_float, func;
};
static_assert(sizeof(WfrArgs) % 8 == 0, "WfrArgs");

__global__ void __launch_bounds__(OB_THREADS) k_wfr_heads(const WfrArgs A_kernarg) {
    HS_KERNARG(WfrArgs, A);
    __shared__ WinS s_wave[OB_WAVES];
    const int64_t j0 = (int64_t)blockIdx.x * OB_TILE + (int64_t)threadIdx.x * WIN_PER;
    uint64_t fwd = 0;
    win_rescan(A.heads, A.carry[blockIdx.x], A.n, s_wave, [&](int k, const WinS run) {
        const int64_t j = j0 + k;
        const uint8_t head = (uint32_t)(j - run.p) % A.width == 0 ? 2 : 0;
        fwd |= (uint64_t)head << (8 * k);
        // position j - 1 ends a block where j starts one, and so does the last row: mirrored, those are the heads
        if (j > 0) A.bheads[1][A.n - j] = head;
        else A.bheads[1][0] = 2;
    });
    if (j0 < A.n) *(uint64_t*)(A.bheads[0] + j0) = fwd;  // whole tiles: the bytes past the rows are not looked at
}

// the cells of the lane's WIN_PER scan positions in direction `dir` (1: mirrored), zero past the rows
__device__ __forceinline__ void wfr_cells(const WfrArgs& A, int dir, uint32_t* s_v, uint32_t (&cell)[WIN_PER]) {
    const int tid = threadIdx.x;
    const int64_t tile0 = (int64_t)blockIdx.x * OB_TILE;
#pragma unroll
    for (int k = 0; k < WIN_PER; ++k) {
        const int e = k * OB_THREADS + tid;
        const int64_t t = tile0 + e;
        s_v[win_get_at(e)] = t < A.n ? A.sorted[dir ? A.n - 1 - t : t] : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < WIN_PER; ++k) cell[k] = s_v[win_put_at(tid, k)];
}

__global__ void __launch_bounds__(OB_THREADS) k_wfr_reduce(const WfrArgs A_kernarg) {
    HS_KERNARG(WfrArgs, A);
    __shared__ WinA s_wave[OB_WAVES];
    __shared__ uint32_t s_v[OB_TILE + OB_THREADS];
    const int dir = blockIdx.y;
    const WinAOps o{A.op};
    uint32_t cell[WIN_PER];
    wfr_cells(A, dir, s_v, cell);
    const WinLane L = win_lane(A.bheads[dir], A.n);
    uint64_t x[WIN_PER];
    wa_lift_lane(o.op, A.is_float, L, [&](int k) { return cell[k]; }, x);
    WinA total;
    win_block_excl(o, win_fold_lane(o, L, [&](int k) { return x[k]; }), s_wave, total);
    if (threadIdx.x == 0) A.tiles[dir][blockIdx.x] = total;
}

__global__ void __launch_bounds__(OB_THREADS) k_wfr_scan(const WfrArgs A_kernarg) {
    HS_KERNARG(WfrArgs, A);
    __shared__ WinA s_wave[OB_WAVES];
    __shared__ uint32_t s_v[OB_TILE + OB_THREADS];
    const int dir = blockIdx.y;
    const WinAOps o{A.op};
    uint32_t cell[WIN_PER];
    wfr_cells(A, dir, s_v, cell);
    const WinLane L = win_lane(A.bheads[dir], A.n);
    uint64_t x[WIN_PER];
    wa_lift_lane(o.op, A.is_float, L, [&](int k) { return cell[k]; }, x);
    uint64_t* tab = A.tab[dir];
    win_rescan_lane(o, L, [&](int k) { return x[k]; }, A.tiles[dir][blockIdx.x], s_wave, [&](int k, const WinA run) {
        const int64_t t = L.j0 + k;  // a row: t < n
        tab[dir ? A.n - 1 - t : t] = run.a;
    });
}

__global__ void __launch_bounds__(OB_THREADS) k_wfr_emit(const WfrArgs A_kernarg) {
    HS_KERNARG(WfrArgs, A);
    __shared__ WinS s_wave[OB_WAVES];
    __shared__ int32_t s_p[OB_TILE + OB_THREADS];
    const int tid = threadIdx.x;
    const int64_t tile0 = (int64_t)blockIdx.x * OB_TILE;
    win_rescan(A.heads, A.carry[blockIdx.x], A.n, s_wave, [&](int k, const WinS run) { s_p[win_put_at(tid, k)] = run.p; });
    __syncthreads();
    uint32_t err = 0;
#pragma unroll
    for (int k = 0; k < WIN_PER; ++k) {
        const int e = k * OB_THREADS + tid;
        const int64_t j = tile0 + e;
        if (j < A.n) {
            const int64_t row = A.perm ? A.perm[j] : j;
            const int64_t p = s_p[win_get_at(e)], last = p + A.part_rows[p] - 1;  // p <= j <= last < n
            const int64_t lo = j - A.preceding > p ? j - A.preceding : p, hi = j + A.following < last ? j + A.following : last;
            uint64_t a = 0;
            if (A.op != WA_NONE) {
                const uint32_t at = (uint32_t)(lo - p), block = at / A.width;
                if ((uint64_t)(hi - p) >= ((uint64_t)block + 1) * A.width) a = wa_op(A.op, A.tab[1][lo], A.tab[0][hi]);
                else a = at == block * A.width ? A.tab[0][hi] : A.tab[1][lo];
            }
            A.out[row] = wa_finish(A.func, A.is_float, a, (int32_t)(hi - lo + 1), err);
        }
    }
    if (err && A.flags) atomicOr(A.flags, err);
}

// -----------------------------------------------------------------------------------------------------
// The host side of the four entries: one workspace layout, one item table, one run routine.
// -----------------------------------------------------------------------------------------------------
// Where everything lies behind the sort's workspace, and where each entry's share of it ends: hs_window's, then what
// hs_window_agg adds, then what hs_window_nav adds, then what hs_window_frames adds.  The items of a call run one after
// the other over the same regions.
struct WinLayout {
    size_t heads;    // a head byte per sorted position, whole tiles
    size_t recs;     // a (p, q, d) record per tile, and one more
    size_t rank_end;
    size_t cells4;   // an argument's 4-byte cells by sorted position, whole tiles
    size_t tab_a;    // a frame's fold ...
    size_t tab_c;    // ... and its rows, by the frame's start position
    size_t recs_a;   // a WinA record per tile, and one more
    size_t agg_end;
    size_t cells8;   // an argument's cells by sorted position at 8 bytes, whole tiles
    size_t ends[2];  // the frames' rows by their start position: PARTITION, RANGE
    size_t nav_end;
    size_t bheads[2];  // sliding frames: block heads by position, block ends by mirrored position, whole tiles
    size_t suf;        // ... the backward fold by position (the forward one lies in tab_a)
    size_t recs_b;     // ... a WinA record per tile of the backward scan, and one more (the forward ones in recs_a)
    size_t frames_end;
};
static_assert(HS_WIN_FRAME_PARTITION == 0 && HS_WIN_FRAME_RANGE == 1, "the end tables are indexed by frame");
static WinLayout win_layout(int64_t nrows) {
    const size_t tiles = (size_t)((nrows + OB_TILE - 1) / OB_TILE), whole = rx_align(tiles * OB_TILE);
    size_t at = 0;
    const auto take = [&at](size_t bytes) {
        const size_t here = at;
        at += bytes;
        return here;
    };
    WinLayout L;
    L.heads = take(whole);
    L.recs = take(rx_align((tiles + 1) * sizeof(WinRec)));
    L.rank_end = at;
    L.cells4 = take(4 * whole);
    L.tab_a = take(rx_align((size_t)nrows * 8));
    L.tab_c = take(rx_align((size_t)nrows * 4));
    L.recs_a = take(rx_align((tiles + 1) * sizeof(WinA)));
    L.agg_end = at;
    L.cells8 = take(8 * whole);
    L.ends[HS_WIN_FRAME_PARTITION] = take(rx_align((size_t)nrows * 4));
    L.ends[HS_WIN_FRAME_RANGE] = take(rx_align((size_t)nrows * 4));
    L.nav_end = at;
    L.bheads[0] = take(whole);
    L.bheads[1] = take(whole);
    L.suf = take(rx_align((size_t)nrows * 8));
    L.recs_b = take(rx_align((tiles + 1) * sizeof(WinA)));
    L.frames_end = at;
    return L;
}

// the sort's workspace, then the layout up to an entry's end
static size_t win_ws_bytes(int64_t nrows, int32_t n_keys, int32_t max_key_words, size_t WinLayout::*end) {
    return nrows < 0 ? 0 : hs_order_by_ws_bytes(nrows, n_keys, max_key_words) + win_layout(nrows).*end;
}
extern "C" size_t hs_window_ws_bytes(int64_t nrows, int32_t n_keys, int32_t max_key_words) {
    return win_ws_bytes(nrows, n_keys, max_key_words, &WinLayout::rank_end);
}
extern "C" size_t hs_window_agg_ws_bytes(int64_t nrows, int32_t n_keys, int32_t max_key_words, int32_t) {
    return win_ws_bytes(nrows, n_keys, max_key_words, &WinLayout::agg_end);
}
extern "C" size_t hs_window_nav_ws_bytes(int64_t nrows, int32_t n_keys, int32_t max_key_words, int32_t) {
    return win_ws_bytes(nrows, n_keys, max_key_words, &WinLayout::nav_end);
}
extern "C" size_t hs_window_frames_ws_bytes(int64_t nrows, int32_t n_keys, int32_t max_key_words, int32_t) {
    return win_ws_bytes(nrows, n_keys, max_key_words, &WinLayout::frames_end);
}

// What an item of each HS_WIN_* code takes beside the keys
enum { WI_ARG_NONE = 0, WI_ARG_32 = 1, WI_ARG_32_64 = 2 };        // the argument column's cells
enum { WI_PARAM_NONE = 0, WI_PARAM_OFFSET = 1, WI_PARAM_BUCKETS = 2 };  // params[i] (an offset comes with a default cell)
struct WinItem {
    uint8_t frame, arg, param;
};
static const WinItem WIN_ITEMS[] = {
    {0, WI_ARG_NONE, WI_PARAM_NONE},     // HS_WIN_ROW_NUMBER
    {0, WI_ARG_NONE, WI_PARAM_NONE},     // HS_WIN_RANK
    {0, WI_ARG_NONE, WI_PARAM_NONE},     // HS_WIN_DENSE_RANK
    {1, WI_ARG_NONE, WI_PARAM_NONE},     // HS_WIN_COUNT
    {1, WI_ARG_32, WI_PARAM_NONE},       // HS_WIN_SUM
    {1, WI_ARG_32, WI_PARAM_NONE},       // HS_WIN_AVG
    {1, WI_ARG_32, WI_PARAM_NONE},       // HS_WIN_MIN
    {1, WI_ARG_32, WI_PARAM_NONE},       // HS_WIN_MAX
    {0, WI_ARG_32_64, WI_PARAM_OFFSET},  // HS_WIN_LAG
    {0, WI_ARG_32_64, WI_PARAM_OFFSET},  // HS_WIN_LEAD
    {1, WI_ARG_32_64, WI_PARAM_NONE},    // HS_WIN_FIRST_VALUE
    {1, WI_ARG_32_64, WI_PARAM_NONE},    // HS_WIN_LAST_VALUE
    {0, WI_ARG_NONE, WI_PARAM_BUCKETS},  // HS_WIN_NTILE
};
static_assert(sizeof(WIN_ITEMS) / sizeof(WIN_ITEMS[0]) == HS_WIN_NTILE + 1 && HS_WIN_COUNT == 3 && HS_WIN_MAX == 7 &&
                  HS_WIN_LAG == 8 && HS_WIN_LAST_VALUE == 11, "WIN_ITEMS is indexed by HS_WIN_*");
static const struct {
    bool i64;                    // HS_I32 and HS_F32 cells, and these?
    const char *others, *takes;  // the refusal's words
} WIN_ARGS[] = {{false, "", ""},
                {false, "a narrow or virtual column, or another type", "HS_I32 or HS_F32"},
                {true, "a narrow or virtual column, a STRING, or another type", "HS_I32, HS_F32 or HS_I64"}};

// What all entries refuse before anything is launched or any device pointer is read, under the caller's name.  HS_OK: go
// on (nrows == 0 included - the caller returns then).
static int win_refuse(const char* name, const hs_col* keys, int32_t n_part, int32_t n_keys, int64_t nrows, const int32_t* funcs,
                      int32_t n_funcs, const void* out, int32_t max_func) {
    if (n_keys < 0 || n_part < 0 || n_part > n_keys || nrows < 0 || n_funcs <= 0 || !funcs || !out) {
        hs_set_error("%s: bad arguments", name);
        return HS_E_ARG;
    }
    if (const int rc = ob_refuse_keys(name, keys, n_keys, "partition and order columns"); rc != HS_OK) return rc;
    if (n_funcs > HS_WIN_MAX_FUNCS) {
        hs_set_error("%s: more than %d functions in one call", name, HS_WIN_MAX_FUNCS);
        return HS_E_LIMIT;
    }
    if (nrows >= (1ll << 31)) {
        hs_set_error("%s: %lld rows; the INTEGER result holds positions below 2^31", name, (long long)nrows);
        return HS_E_LIMIT;
    }
    for (int f = 0; f < n_funcs; ++f) {
        if (funcs[f] < 0 || funcs[f] > max_func) {
            hs_set_error("%s: function %d is not one of HS_WIN_*", name, funcs[f]);
            return HS_E_ARG;
        }
        if ((funcs[f] == HS_WIN_RANK || funcs[f] == HS_WIN_DENSE_RANK) && n_part == n_keys) {
            hs_set_error("%s: RANK / DENSE_RANK need an order key", name);
            return HS_E_ARG;
        }
    }
    return HS_OK;
}

// Does item i slide (HS_WIN_FRAME_BETWEEN, in the entry that takes it: the others do not look at the frame of a function
// without one), and which of the frame's two offsets does it read?  FIRST_VALUE looks at the frame's first row only,
// LAST_VALUE at its last.
static bool win_slides(int32_t max_frame, const int32_t* frames, int i) {
    return max_frame == HS_WIN_FRAME_BETWEEN && frames && frames[i] == HS_WIN_FRAME_BETWEEN;
}
static bool win_reads_preceding(int32_t func) { return func != HS_WIN_LAST_VALUE; }
static bool win_reads_following(int32_t func) { return func != HS_WIN_FIRST_VALUE; }

// What item i needs by WIN_ITEMS, behind win_refuse: its frame (up to the entry's `max_frame`) and a sliding frame's
// offsets, its parameter, its argument's kind, in this order.  Nothing is launched, no device pointer read.
static int win_refuse_item(const char* name, int i, const int32_t* funcs, const int32_t* frames, int32_t max_frame,
                           const hs_col* values, const int64_t* params, const uint64_t* defaults, const int64_t* preceding,
                           const int64_t* following) {
    const WinItem& item = WIN_ITEMS[funcs[i]];
    if (item.frame && (!frames || frames[i] < HS_WIN_FRAME_PARTITION || frames[i] > max_frame)) {
        hs_set_error("%s: item %d: frame %d is not one of HS_WIN_FRAME_*", name, i, frames ? frames[i] : -1);
        return HS_E_ARG;
    }
    if (win_slides(max_frame, frames, i)) {
        if (!item.frame) {
            hs_set_error("%s: item %d: frame %d on function %d, which takes no frame", name, i, frames[i], funcs[i]);
            return HS_E_ARG;
        }
        const struct {
            bool read;
            const int64_t* at;
            const char* what;
        } ends[2] = {{win_reads_preceding(funcs[i]), preceding, "preceding"}, {win_reads_following(funcs[i]), following, "following"}};
        for (const auto& end : ends) {
            if (!end.read) continue;
            if (!end.at) {
                hs_set_error("%s: item %d: frame %d needs its offset (%s is null)", name, i, frames[i], end.what);
                return HS_E_ARG;
            }
            if (end.at[i] < 0 || end.at[i] >= (1ll << 31)) {
                hs_set_error("%s: item %d: %s is %lld; it lies in [0, 2^31)", name, i, end.what, (long long)end.at[i]);
                return HS_E_ARG;
            }
        }
    }
    if (item.param != WI_PARAM_NONE) {
        const int64_t least = item.param == WI_PARAM_BUCKETS ? 1 : 0;
        const char* what = item.param == WI_PARAM_BUCKETS ? "the bucket count n" : "the offset k";
        if (!params) {
            hs_set_error("%s: item %d: %s is missing (params is null)", name, i, what);
            return HS_E_ARG;
        }
        if (params[i] < least || params[i] >= (1ll << 31)) {
            hs_set_error("%s: item %d: %s is %lld; it lies in [%lld, 2^31)", name, i, what, (long long)params[i], (long long)least);
            return HS_E_ARG;
        }
        if (item.param == WI_PARAM_OFFSET && !defaults) {
            hs_set_error("%s: item %d: LAG / LEAD need a default cell (defaults is null)", name, i);
            return HS_E_ARG;
        }
    }
    if (item.arg != WI_ARG_NONE) {
        const auto& arg = WIN_ARGS[item.arg];
        const int32_t kind = values ? values[i].kind : -1;
        if (kind != HS_I32 && kind != HS_F32 && !(arg.i64 && kind == HS_I64)) {
            hs_set_error("%s: item %d: the argument is a column of kind %d (%s); it takes %s cells", name, i, kind, arg.others,
                         arg.takes);
            return HS_E_ARG;
        }
    }
    return HS_OK;
}

// The four entries: `max_func` / `max_frame` the highest HS_WIN_* / HS_WIN_FRAME_* code the entry takes, `last` what it calls
// its launches behind the front half; an entry passes null for the arrays it does not have.  ONE sort, ONE heads pass and ONE (p, q, d) tile carry for
// all items of a call, then the items one after the other.  An entry's workspace ends with its share of WinLayout:
// pointers into the regions behind it are formed here and not used, no item of the entry reaching them.
static int win_run(const char* name, const char* last, int32_t max_func, int32_t max_frame, void* stream_, const hs_col* keys,
                   const int32_t* descending, int32_t n_part, int32_t n_keys, int64_t nrows, const int32_t* funcs,
                   const int32_t* frames, const hs_col* values, const int64_t* params, const uint64_t* defaults,
                   const int64_t* preceding, const int64_t* following, int32_t n_items, void* const* out, void* ws_,
                   uint32_t* flags) {
    int rc = win_refuse(name, keys, n_part, n_keys, nrows, funcs, n_items, out, max_func);
    if (rc != HS_OK) return rc;
    for (int i = 0; i < n_items; ++i)
        if ((rc = win_refuse_item(name, i, funcs, frames, max_frame, values, params, defaults, preceding, following)) != HS_OK)
            return rc;
    if (nrows == 0) return HS_OK;
    const auto takes_value = [&](int i) { return WIN_ITEMS[funcs[i]].arg != WI_ARG_NONE; };
    for (int i = 0; i < n_items; ++i)
        if (takes_value(i) && !values[i].data) {
            hs_set_error("%s: item %d: the argument column is null", name, i);
            return HS_E_ARG;
        }
    if (!ws_ || (n_keys > 0 && !keys) || (n_keys > n_part && !descending)) {
        hs_set_error("%s: bad arguments", name);
        return HS_E_ARG;
    }
    for (int i = 0; i < n_items; ++i)
        if (!out[i]) {
            hs_set_error("%s: output %d is null", name, i);
            return HS_E_ARG;
        }
    if ((rc = ob_refuse_kinds(name, keys, n_keys, "key", "ordered")) != HS_OK) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    int32_t desc[HS_MAX_COLS] = {0};
    for (int k = n_part; k < n_keys; ++k) desc[k] = descending[k] ? 1 : 0;
    ObSorted S;
    int64_t sorted_rows = 0;
    if ((rc = ob_sort(stream, keys, desc, n_keys, nrows, nullptr, -1, &sorted_rows, ws_, name, S)) != HS_OK) return rc;
    WinHeads H{ob_run(S, n_keys)};  // n: nrows, nothing limits the rows
    for (int k = 0; k < n_part; ++k) H.part_bytes += S.keys.width[k];
    uint8_t* base = (uint8_t*)ws_ + S.ws_bytes;  // behind what the sort laid out
    const WinLayout L = win_layout(nrows);
    H.heads = base + L.heads;
    const WinTile T{H.heads, H.perm, (WinRec*)(base + L.recs), nrows};
    const int64_t tiles = (nrows + OB_TILE - 1) / OB_TILE;
    const dim3 grid((unsigned)tiles), block(OB_THREADS);
    hipLaunchKernelGGL(k_win_heads, grid, block, 0, stream, H);
    if (hipGetLastError() != hipSuccess) {
        hs_set_error("%s (heads): kernel launch failed", name);
        return HS_E_LAUNCH;
    }
    hipLaunchKernelGGL(k_win_reduce, grid, block, 0, stream, T.heads, nrows, (WinRec*)T.carry);
    hipLaunchKernelGGL(k_win_tiles<WinSOps>, dim3(1), block, 0, stream, (WinRec*)T.carry, tiles, WinSOps{});
    if (hipGetLastError() != hipSuccess) {
        hs_set_error("%s (scan): kernel launch failed", name);
        return HS_E_LAUNCH;
    }
    WinEmit E{T};  // the other fields: zero
    WaggArgs A{T};
    WnavArgs N{T};
    A.sorted = (uint32_t*)(base + L.cells4);
    A.tab_a = (uint64_t*)(base + L.tab_a);
    A.tab_c = (int32_t*)(base + L.tab_c);
    A.tiles = (WinA*)(base + L.recs_a);
    A.flags = flags;
    void* sorted = base + L.cells8;
    int32_t* ends[2] = {(int32_t*)(base + L.ends[HS_WIN_FRAME_PARTITION]), (int32_t*)(base + L.ends[HS_WIN_FRAME_RANGE])};
    // the end tables, once per frame some item needs: k_wagg_scan without an argument (its tab_a cells are not used)
    bool needed[2] = {false, false};
    for (int i = 0; i < n_items; ++i) {
        if (funcs[i] == HS_WIN_LEAD || funcs[i] == HS_WIN_NTILE) needed[HS_WIN_FRAME_PARTITION] = true;
        if (win_slides(max_frame, frames, i)) needed[HS_WIN_FRAME_PARTITION] |= funcs[i] != HS_WIN_FIRST_VALUE;  // the frame's clamp
        else if (funcs[i] == HS_WIN_LAST_VALUE && frames[i] != HS_WIN_FRAME_ROWS) needed[frames[i]] = true;
    }
    WfrArgs F{T};
    F.part_rows = ends[HS_WIN_FRAME_PARTITION];
    F.bheads[0] = base + L.bheads[0], F.bheads[1] = base + L.bheads[1];
    F.tiles[0] = A.tiles, F.tiles[1] = (WinA*)(base + L.recs_b);
    F.tab[0] = A.tab_a, F.tab[1] = (uint64_t*)(base + L.suf);
    F.flags = flags;
    const dim3 both((unsigned)tiles, 2);  // the forward and the backward scan of a sliding item
    for (int fr = HS_WIN_FRAME_PARTITION; fr <= HS_WIN_FRAME_RANGE; ++fr) {
        if (!needed[fr]) continue;
        WaggArgs Ends = A;
        Ends.op = WA_NONE;
        Ends.frame = fr;
        Ends.tab_c = ends[fr];
        hipLaunchKernelGGL(k_wagg_scan, grid, block, 0, stream, Ends);
    }
    uint32_t done = 0;
    for (int i = 0; i < n_items; ++i) {
        if (done & (1u << i)) continue;
        const int32_t func = funcs[i], frame = frames ? frames[i] : 0;
        if (func < HS_WIN_COUNT || (func == HS_WIN_COUNT && frame == HS_WIN_FRAME_ROWS)) {
            E.out = (int32_t*)out[i];
            E.func = func < HS_WIN_COUNT ? func : HS_WIN_ROW_NUMBER;  // the rows from the partition's first through this one
            hipLaunchKernelGGL(k_win_emit, grid, block, 0, stream, E);
            continue;
        }
        if (func <= HS_WIN_MAX && win_slides(max_frame, frames, i)) {
            F.func = func;
            F.out = (uint32_t*)out[i];
            F.preceding = preceding[i], F.following = following[i];
            F.op = WA_NONE;
            if (func != HS_WIN_COUNT) {
                const int64_t w = preceding[i] + following[i] + 1;  // up to 2^32 - 1
                const uint32_t width = (uint32_t)(w < (1ll << 31) ? w : (1ll << 31));
                if (width != F.width) {  // the head bytes of the item before hold for the same W
                    F.width = width;
                    hipLaunchKernelGGL(k_wfr_heads, grid, block, 0, stream, F);
                }
                F.is_float = values[i].kind == HS_F32;
                F.op = func == HS_WIN_MIN ? WA_MIN : func == HS_WIN_MAX ? WA_MAX : F.is_float ? WA_ADD_F : WA_ADD_I;
                F.sorted = (const uint32_t*)values[i].data;
                if (T.perm) {
                    F.sorted = A.sorted;
                    hipLaunchKernelGGL(k_wnav_gather<uint32_t>, grid, block, 0, stream, T.perm, (const uint32_t*)values[i].data,
                                       A.sorted, nrows);
                }
                hipLaunchKernelGGL(k_wfr_reduce, both, block, 0, stream, F);
                hipLaunchKernelGGL(k_win_tiles<WinAOps>, dim3(1), block, 0, stream, F.tiles[0], tiles, WinAOps{F.op});
                hipLaunchKernelGGL(k_win_tiles<WinAOps>, dim3(1), block, 0, stream, F.tiles[1], tiles, WinAOps{F.op});
                hipLaunchKernelGGL(k_wfr_scan, both, block, 0, stream, F);
            }
            hipLaunchKernelGGL(k_wfr_emit, grid, block, 0, stream, F);
            continue;
        }
        if (func <= HS_WIN_MAX) {
            A.func = func;
            A.frame = frame;
            A.out = (uint32_t*)out[i];
            A.op = WA_NONE;
            if (func != HS_WIN_COUNT) {
                A.is_float = values[i].kind == HS_F32;
                A.values = (const uint32_t*)values[i].data;
                A.op = func == HS_WIN_MIN ? WA_MIN : func == HS_WIN_MAX ? WA_MAX : A.is_float ? WA_ADD_F : WA_ADD_I;
                hipLaunchKernelGGL(k_wagg_reduce, grid, block, 0, stream, A);
                hipLaunchKernelGGL(k_win_tiles<WinAOps>, dim3(1), block, 0, stream, A.tiles, tiles, WinAOps{A.op});
            }
            hipLaunchKernelGGL(k_wagg_scan, grid, block, 0, stream, A);
            hipLaunchKernelGGL(k_wagg_emit, grid, block, 0, stream, A);
            continue;
        }
        const bool wide = takes_value(i) && values[i].kind == HS_I64;
        if (takes_value(i)) {  // the argument in sorted order, once for every item that reads the same cells
            N.cells = values[i].data;
            if (T.perm) {
                N.cells = sorted;
                if (wide)
                    hipLaunchKernelGGL(k_wnav_gather<uint64_t>, grid, block, 0, stream, T.perm, (const uint64_t*)values[i].data,
                                       (uint64_t*)sorted, nrows);
                else
                    hipLaunchKernelGGL(k_wnav_gather<uint32_t>, grid, block, 0, stream, T.perm, (const uint32_t*)values[i].data,
                                       (uint32_t*)sorted, nrows);
            }
        }
        for (int t = i; t < n_items; ++t) {  // this item, then the later navigation items over the same argument
            if (t > i && (!takes_value(i) || funcs[t] < HS_WIN_LAG || !takes_value(t) || (done & (1u << t)) ||
                          values[t].data != values[i].data || (values[t].kind == HS_I64) != wide))
                continue;
            done |= 1u << t;
            N.func = funcs[t];
            N.frame = frames ? frames[t] : 0;
            N.k = params ? params[t] : 0;
            if (win_slides(max_frame, frames, t)) N.k = N.func == HS_WIN_FIRST_VALUE ? preceding[t] : following[t];
            N.dflt = defaults ? defaults[t] : 0;
            N.tab_c = ends[N.func == HS_WIN_LAST_VALUE && N.frame == HS_WIN_FRAME_RANGE ? 1 : 0];
            N.out = out[t];
            if (wide) hipLaunchKernelGGL(k_wnav_emit<uint64_t>, grid, block, 0, stream, N);
            else hipLaunchKernelGGL(k_wnav_emit<uint32_t>, grid, block, 0, stream, N);
        }
    }
    if (hipGetLastError() != hipSuccess) {
        hs_set_error("%s (%s): kernel launch failed", name, last);
        return HS_E_LAUNCH;
    }
    return HS_OK;
}

extern "C" int hs_window(void* stream, const hs_col* keys, const int32_t* descending, int32_t n_part, int32_t n_keys,
                         int64_t nrows, const int32_t* funcs, int32_t n_funcs, int32_t* const* out, void* ws, uint32_t* flags) {
    return win_run("hs_window", "emit", HS_WIN_DENSE_RANK, HS_WIN_FRAME_ROWS, stream, keys, descending, n_part, n_keys, nrows, funcs,
                   nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, n_funcs, (void* const*)out, ws, flags);
}
extern "C" int hs_window_agg(void* stream, const hs_col* keys, const int32_t* descending, int32_t n_part, int32_t n_keys,
                             int64_t nrows, const int32_t* funcs, const int32_t* frames, const hs_col* values, int32_t n_items,
                             void* const* out, void* ws, uint32_t* flags) {
    return win_run("hs_window_agg", "items", HS_WIN_MAX, HS_WIN_FRAME_ROWS, stream, keys, descending, n_part, n_keys, nrows, funcs,
                   frames, values, nullptr, nullptr, nullptr, nullptr, n_items, out, ws, flags);
}
extern "C" int hs_window_nav(void* stream, const hs_col* keys, const int32_t* descending, int32_t n_part, int32_t n_keys,
                             int64_t nrows, const int32_t* funcs, const int32_t* frames, const hs_col* values,
                             const int64_t* params, const uint64_t* defaults, int32_t n_items, void* const* out, void* ws,
                             uint32_t* flags) {
    return win_run("hs_window_nav", "items", HS_WIN_NTILE, HS_WIN_FRAME_ROWS, stream, keys, descending, n_part, n_keys, nrows, funcs,
                   frames, values, params, defaults, nullptr, nullptr, n_items, out, ws, flags);
}
extern "C" int hs_window_frames(void* stream, const hs_col* keys, const int32_t* descending, int32_t n_part, int32_t n_keys,
                                int64_t nrows, const int32_t* funcs, const int32_t* frames, const hs_col* values,
                                const int64_t* params, const uint64_t* defaults, const int64_t* preceding,
                                const int64_t* following, int32_t n_items, void* const* out, void* ws, uint32_t* flags) {
    return win_run("hs_window_frames", "items", HS_WIN_NTILE, HS_WIN_FRAME_BETWEEN, stream, keys, descending, n_part, n_keys, nrows,
                   funcs, frames, values, params, defaults, preceding, following, n_items, out, ws, flags);
}

// out[i] = values[s] for bounds[s] <= i < bounds[s + 1]: a value per segment spread over the segment's rows (the global
// block id of every partial row, multi-rank partial aggregate).  Replaces torch.repeat_interleave.
__global__ void __launch_bounds__(256) k_expand_by_bounds(const int64_t* bounds, const int64_t* values, int64_t n_seg, int64_t n,
                                                          int64_t* out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t lo = 0, hi = n_seg;  // last s with bounds[s] <= i
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (bounds[mid] <= i) lo = mid;
            else hi = mid;
        }
        out[i] = values[lo];
    }
}
extern "C" int hs_expand_by_bounds(void* stream, const int64_t* bounds, const int64_t* values, int64_t n_seg, int64_t n, int64_t* out) {
    if (n == 0) return HS_OK;
    if (!bounds || !values || !out || n_seg < 1 || n < 0) {
        hs_set_error("hs_expand_by_bounds: bad arguments");
        return HS_E_ARG;
    }
    hipLaunchKernelGGL(k_expand_by_bounds, dim3((unsigned)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, bounds, values, n_seg, n, out);
    RX_CHECK_LAUNCH("hs_expand_by_bounds");
    return HS_OK;
}

// =====================================================================================================
// The general inner join on INTEGER keys over a dense key range (round 4; include/hipspark.h hs_join_dense_*)
// =====================================================================================================
// Reference: BroadcastHashJoinTask.generate_chunks tasks.py:201-240 - a hash map key -> build rows (in row order), every
// probe row emits its matches in that order; duplicates on either side multiply (zig twin: tasks.zig:70-194, 258-326).
// Round 1-3 built one open-addressing table over all build keys with a 64-bit atomic per row scattered over 800 MB
// (8.6 G keys/s, 5.6 % of the HBM roofline).  Here the build side is MOVED instead, like the radix tier of GROUP BY:
//   1. two stable partition passes (the kernels above, RX_BIN_RANGE) on the most significant bits of slot = key - key_min
//      bring the (key, row) tuples into partitions of 2^L consecutive slots, still in row order;
//   2. one wave per partition (k_jd_assemble): slot counts in LDS, a scan, then the rows are placed IN ORDER - lanes of a
//      64-tuple step that share a slot rank themselves with ballots - so every slot's rows come out ascending without a
//      sort and without a global atomic; the partition's slice of starts[] (CSR offsets, one per SLOT, absent keys
//      included) leaves with coalesced stores.
// The probe is then one or two adjacent 4-byte reads per row (starts[s], starts[s + 1]) instead of a hash probe over
// three arrays: count -> exclusive scan -> fill, pairs ordered by probe row, then build row (tasks.py:224-240).
// The hashed INTEGER and STRING forms below share this build (jx_* : partition passes, per-window assembly, probe epilogue).
constexpr int JD_MAX_L = 13;  // slots of one partition: 2^L cursors + 2^L first rows (uint32) + 2^L tag bytes in LDS per wave (72 KB at most)
constexpr uint32_t JD_EMPTY = 0xffffffffu;  // slot word: no build row has this key
constexpr uint32_t JD_MULTI = 0x80000000u;  // slot word: several - the low 31 bits are the start of the key's list in rows[]

// ---- the assembly of one partition (dense) or window (hashed), one wave each --------------------------------------------
// The wave walks its tuples [b, e) in row order with LDS tables of 2^L slots: cur[] (counts, then list cursors), head[] (the
// first = lowest build row of every slot) and tag[] (placement: the lane that came by last in this step).  L is a
// compile-time constant in the hashed kernels and a run-time value in the dense one; the helpers take it as an argument.

// Clears the tables (and what clear(s) adds), then every tuple claims its slot - claim(tuple, i) -> slot, < 0: none, the
// window is full - and counts a row there (LDS atomics: counting is order-free).  load(i) fetches tuple i; the first
// step's tuples are asked for before the tables are cleared, every later step's before the current one is worked on (a
// wave walks its partition in order: without this it paid one global round trip per step).  -> a tuple of this lane found
// no slot.
template <typename Load, typename Clear, typename Claim>
__device__ __forceinline__ bool jx_count(uint32_t* cur, uint32_t* head, int L, int64_t b, int64_t e, int lane, Load load, Clear clear,
                                         Claim claim) {
    decltype(load(b)) next{};
    if (b + lane < e) next = load(b + lane);
    for (int s = lane; s < (1 << L); s += HS_WAVE) {
        clear(s);
        cur[s] = 0;
        head[s] = JD_EMPTY;
    }
    rx_wave_handover();
    bool full = false;
    for (int64_t base = b; base < e; base += HS_WAVE) {
        const auto t = next;
        const bool valid = base + lane < e;
        if (base + HS_WAVE + lane < e) next = load(base + HS_WAVE + lane);
        if (valid) {
            const int s = claim(t, base + lane);
            if (s < 0) full = true;
            else atomicAdd(&cur[s], 1u);
        }
    }
    rx_wave_handover();
    return full;
}

// exclusive scan of the 2^L counts: a lane's consecutive slots, then a scan over the lanes
__device__ __forceinline__ void jx_scan(uint32_t* cur, int L, int lane) {
    const int per = (1 << L) / HS_WAVE;  // (2^L >= 64)
    uint32_t sum = 0;
    for (int k = 0; k < per; ++k) sum += cur[lane * per + k];
    uint32_t x = sum;
    for (int d = 1; d < HS_WAVE; d <<= 1) {
        const uint32_t up = __shfl_up(x, d, HS_WAVE);
        if (lane >= d) x += up;
    }
    uint32_t run = x - sum;
    for (int k = 0; k < per; ++k) {
        const uint32_t c = cur[lane * per + k];
        cur[lane * per + k] = run;
        run += c;
    }
    rx_wave_handover();
}

// Ordered placement of the build rows rows[b, e) into out_rows[b, e): tuples arrive in row order; within a step, equal
// slots take consecutive places in lane order.  Usually the 64 tuples of a step fall into 64 DIFFERENT slots (unique or
// nearly unique build keys): every lane leaves its number in a tag byte of its slot and reads it back - all lanes find
// their own: no ranking needed (the ten ballots per step were a third of this kernel).  Tuple i's slot is
// slot(load(i)): the load is prefetched a step ahead, the slot worked out when the step comes.
template <typename Load, typename Slot>
__device__ __forceinline__ void jx_place(uint32_t* cur, uint32_t* head, uint8_t* tag, int L, int64_t b, int64_t e, int lane, Load load,
                                         Slot slot, const uint32_t* rows, uint32_t* out_rows) {
    const uint64_t below = (1ull << lane) - 1ull;
    decltype(load(b)) nt{};
    uint32_t nrow = 0u;
    if (b + lane < e) {
        nt = load(b + lane);
        nrow = rows[b + lane];
    }
    for (int64_t base = b; base < e; base += HS_WAVE) {
        const bool valid = base + lane < e;
        const uint32_t s = slot(nt), row = nrow;
        if (base + HS_WAVE + lane < e) {
            nt = load(base + HS_WAVE + lane);
            nrow = rows[base + HS_WAVE + lane];
        }
        if (valid) tag[s] = (uint8_t)lane;
        rx_wave_handover();
        const bool shared_slot = valid && tag[s] != (uint8_t)lane;
        const uint32_t at = valid ? cur[s] : 0u;
        const uint32_t first = valid ? head[s] : 0u;
        if (__ballot(shared_slot) == 0) {  // (wave-uniform) 64 different slots: nothing to rank
            if (valid) {
                out_rows[b + at] = row;
                cur[s] = at + 1u;
                if (first == JD_EMPTY) head[s] = row;
            }
            rx_wave_handover();
            continue;
        }
        const uint64_t peers = rx_peers(s, valid, L);
        const uint32_t rank = (uint32_t)__popcll(peers & below);
        rx_wave_handover();  // every lane has read its slot's cursor before a leader moves it
        if (valid) {
            out_rows[b + at + rank] = row;
            if (rank == 0) {
                cur[s] = at + (uint32_t)__popcll(peers);
                if (first == JD_EMPTY) head[s] = row;  // the step's lowest lane of the slot holds its lowest row
            }
        }
        rx_wave_handover();
    }
}

// the words of slots [0, live), store(s, word) (coalesced): JD_EMPTY, the one build row, or JD_MULTI + the list's start, whose
// length goes to list_count there.  Lists lie in SLOT order, so list s starts where list s - 1 ends.
template <typename Store>
__device__ __forceinline__ void jx_emit(const uint32_t* cur, const uint32_t* head, int64_t b, int64_t live, int lane, uint32_t* list_count,
                                        Store store) {
    for (int s = lane; s < live; s += HS_WAVE) {
        const uint32_t end = cur[s], start = s ? cur[s - 1] : 0u;
        const uint32_t c = end - start;
        uint32_t word = JD_EMPTY;
        if (c == 1) word = head[s];
        else if (c > 1) {
            word = JD_MULTI | (uint32_t)(b + start);
            list_count[b + start] = c;
        }
        store(s, word);
    }
    rx_wave_handover();
}

struct JdAssemble {
    const int64_t* seg_start;  // [parts + 1] tuple ranges of the partitions
    int64_t parts;
    const int32_t* keys;       // tuples, partitioned
    const uint32_t* rows;
    int64_t slots;
    int32_t key_min, L;
    uint32_t* words;           // [slots]: JD_EMPTY | the one build row | JD_MULTI + list start
    uint32_t* out_rows;        // [n]: build rows in slot order, ascending within a slot
    uint32_t* list_count;      // [n]: at the start of a list of several rows, its length
    int64_t n;
    uint32_t* flags;
};

__global__ void __launch_bounds__(256) k_jd_assemble(const JdAssemble A) {
    extern __shared__ __align__(16) uint32_t jd_lds[];
    const int lane = threadIdx.x & (HS_WAVE - 1), w = threadIdx.x / HS_WAVE, wpb = blockDim.x / HS_WAVE;
    const int W = 1 << A.L;
    uint32_t* cur = jd_lds + (size_t)w * (2 * W + W / 4);
    uint32_t* head = cur + W;
    uint8_t* tag = (uint8_t*)(head + W);
    const uint32_t wmask = (uint32_t)(W - 1), kmin = (uint32_t)A.key_min;
    const auto key_at = [&](int64_t i) { return A.keys[i]; };
    const auto slot = [=](int32_t key) { return ((uint32_t)key - kmin) & wmask; };
    uint32_t err = 0;
    for (int64_t p = (int64_t)blockIdx.x * wpb + w; p < A.parts; p += (int64_t)gridDim.x * wpb) {
        const int64_t b = A.seg_start[p], e = A.seg_start[p + 1];
        const int64_t slot0 = p << A.L;
        if (slot0 >= A.slots) {
            if (e > b) err |= HS_FLAG_BAD_PROGRAM;  // a key past the declared range
            continue;
        }
        jx_count(cur, head, A.L, b, e, lane, key_at, [](int) {}, [&](int32_t key, int64_t) { return (int)slot(key); });
        jx_scan(cur, A.L, lane);
        jx_place(cur, head, tag, A.L, b, e, lane, key_at, slot, A.rows, A.out_rows);
        // the partition's slice of the slot words
        const int64_t live = A.slots - slot0 < W ? A.slots - slot0 : W;
        jx_emit(cur, head, b, live, lane, A.list_count, [&](int s, uint32_t word) { A.words[slot0 + s] = word; });
    }
    if (err) atomicOr(A.flags, err);
}

// the one segment [0, n) of the first pass; without passes (a key range of one partition) the tuples are the build column
// itself and the row ids 0 .. n-1
__global__ void __launch_bounds__(256) k_jd_setup(uint32_t* iota, int64_t n_iota, int64_t n, int64_t* seg0) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_iota; i += (int64_t)gridDim.x * blockDim.x) iota[i] = (uint32_t)i;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        seg0[0] = 0;
        seg0[1] = n;
    }
}

// ---- the build's host side, shared by the three forms -----------------------------------------------------------------
enum JxForm { JX_DENSE, JX_HASH, JX_HASH_STR, JX_KEYSET };
constexpr int JH_L_SMALL = 9, JH_L_LARGE = 10;  // window sizes of the hashed forms (log2), see their section below

static int64_t jh_windows(int64_t n_build, int L) {   // ~1.75 slots per build row: distinct keys <= rows
    const int64_t w = (n_build * 7 / 4 + ((int64_t)1 << L) - 1) >> L;
    return w < 1 ? 1 : w;
}

struct JxLayout {
    size_t keys_a, rows_a, keys_b, rows_b, iota, slot_of, win, fp, fp_a, fp_b, seg0, seg1, seg2, tb0, tb1, cnt, scan, scan_ws, total;
    int64_t tiles1, tiles2, nseg1, parts, counters, windows;
    int L, bits1, bits2;
};
// Geometry and workspace of a build of n rows.  Dense: partitions of 2^L consecutive slots of the key range `slots`; hashed:
// `windows` windows of 2^L slots.  The partition passes' arrays, then the hashed forms' slot scratch and the STRING form's
// window numbers and fingerprints.
static bool jx_layout(JxForm form, int64_t n, int64_t slots, JxLayout& Y) {
    if (n < 0 || n >= 0x7fffffffll) return false;  // a slot word holds a row in 31 bits
    int bits = 0;
    if (form == JX_DENSE) {
        if (slots < 1 || slots > ((int64_t)1 << 29)) return false;
        int S = 0;
        while (S < 31 && ((int64_t)1 << S) < slots) ++S;
        Y.L = 9;  // 512 slots: 4.5 KB of LDS per wave in the assembly (it runs on the number of waves a CU holds) ...
        if (S - Y.L > 2 * RX_MAX_BITS) Y.L = S - 2 * RX_MAX_BITS;  // ... more when 65 536 partitions would not cover the range
        if (Y.L > JD_MAX_L) return false;  // (slots <= 2^29 with 16 partition bits)
        bits = S > Y.L ? S - Y.L : 0;
        Y.windows = 0;
    } else if (form == JX_KEYSET) {  // keys alone, partitions of 2^L BITS (Y.L is the caller's: ks_partition_bits)
        if (slots < 1 || slots > ((int64_t)1 << 32) || Y.L < 32 - 2 * RX_MAX_BITS || Y.L > 19) return false;
        int S = 0;
        while (S < 32 && ((int64_t)1 << S) < slots) ++S;
        bits = S > Y.L ? S - Y.L : 0;
        Y.windows = 0;
    } else {
        Y.L = jh_windows(n, JH_L_SMALL) <= ((int64_t)1 << (2 * RX_MAX_BITS)) ? JH_L_SMALL : JH_L_LARGE;
        Y.windows = jh_windows(n, Y.L);
        while (((int64_t)1 << bits) < Y.windows) ++bits;
        if (bits > 2 * RX_MAX_BITS) return false;  // 65 536 windows = 38 M build rows per call
    }
    Y.bits1 = bits <= RX_MAX_BITS ? bits : (bits + 1) / 2;
    Y.bits2 = bits - Y.bits1;
    Y.nseg1 = (int64_t)1 << Y.bits1;
    Y.parts = (int64_t)1 << bits;
    Y.tiles1 = n / RX_TILE + 2;
    Y.tiles2 = Y.bits2 ? n / RX_TILE + Y.nseg1 + 1 : 0;
    const int64_t c1 = Y.tiles1 << Y.bits1, c2 = Y.tiles2 << Y.bits2;
    Y.counters = c1 > c2 ? c1 : c2;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += rx_align(bytes);
        return at;
    };
    const size_t col = (size_t)n * 4 + 64;  // one 4-byte column
    const bool str = form == JX_HASH_STR, set = form == JX_KEYSET;  // a key set moves no row ids and keeps no copy without a pass
    Y.keys_a = take(set && !Y.bits1 ? 0 : col);
    Y.rows_a = take(set ? 0 : col);
    Y.keys_b = take(Y.bits2 ? col : 0);
    Y.rows_b = take(Y.bits2 && !set ? col : 0);
    Y.iota = take(Y.bits1 || set ? 64 : col);  // row ids travel from the first pass on; needed as an array only without passes
    Y.slot_of = take(form == JX_DENSE || set ? 0 : (size_t)n * 2 + 64);
    Y.win = take(str ? col : 0);
    Y.fp = take(str ? col : 0);
    Y.fp_a = take(str && Y.bits1 ? col : 0);
    Y.fp_b = take(str && Y.bits2 ? col : 0);
    Y.seg0 = take(16);
    Y.seg1 = take((size_t)(Y.nseg1 + 1) * 8);
    Y.seg2 = take((size_t)(Y.parts + 1) * 8);
    Y.tb0 = take(16);
    Y.tb1 = take((size_t)(Y.nseg1 + 1) * 8);
    Y.cnt = take((size_t)Y.counters * 8);
    Y.scan = take((size_t)(Y.counters + 1) * 8);
    Y.scan_ws = take(hs_scan_ws_bytes(Y.counters > 1 ? Y.counters : 1));
    Y.total = off;
    return true;
}

// what one assembly launch reads: (partition key, row id[, third column]) tuples in partition order, and their ranges
struct JxTuples {
    const void* keys;
    const uint32_t* rows;
    const uint32_t* third;
    const int64_t* seg;  // [parts + 1]
    int64_t parts;
};
// Row ids, then one or two stable partition passes (RxPass.mode = mode, range_bias = bias) on the bits1 + bits2 bits of
// the 4-byte partition key `key` above bit `low`; `third` (4 bytes per row, or null) travels along.  Without passes (one
// partition) the tuples are the columns themselves and the row ids 0 .. n-1; without rows every partition is empty.
// with_rows = false (a key set): the keys travel ALONE - no row id column is made, moved or written (T.rows is null).
static int jx_partition(hipStream_t stream, const char* who, uint8_t* ws, const JxLayout& Y, int64_t n, const void* key, RxBin mode,
                        int32_t bias, int low, const uint32_t* third, JxTuples& T, bool with_rows = true) {
    uint32_t* iota = (uint32_t*)(ws + Y.iota);
    int64_t* seg0 = (int64_t*)(ws + Y.seg0);
    int64_t* seg1 = (int64_t*)(ws + Y.seg1);
    int64_t* seg2 = (int64_t*)(ws + Y.seg2);
    const int64_t n_iota = Y.bits1 || !with_rows ? 0 : n;
    int64_t grid = (n_iota + 255) / 256;
    grid = grid < 1 ? 1 : (grid > 4096 ? 4096 : grid);
    hipLaunchKernelGGL(k_jd_setup, dim3((unsigned)grid), dim3(256), 0, stream, iota, n_iota, n, seg0);
    if (hipGetLastError() != hipSuccess) {
        hs_set_error("%s (row ids): kernel launch failed", who);
        return HS_E_LAUNCH;
    }
    T = JxTuples{key, with_rows ? iota : nullptr, third, seg0, 1};
    if (Y.bits1 == 0) return HS_OK;
    T.seg = seg2;
    T.parts = Y.parts;
    if (n == 0) {  // no rows: every partition is empty
        hs_memset_async(seg2, 0, (size_t)(Y.parts + 1) * 8, stream);
        return HS_OK;
    }
    RxPass P;
    std::memset(&P, 0, sizeof(P));
    P.n_cols = !with_rows ? 1 : third ? 3 : 2;
    P.esize[0] = P.esize[1] = 4;
    if (third) P.esize[2] = 4;
    P.mode = mode;
    P.range_bias = bias;
    P.key = hs_col{HS_I32, -1, key, nullptr, nullptr};
    P.row0 = 0;
    // pass 1: the top bits1 bits over the one segment [0, n)
    P.seg_start = seg0;
    P.tile_base = (int64_t*)(ws + Y.tb0);
    P.n_seg = 1;
    P.shift = low + Y.bits2;
    P.bits = Y.bits1;
    P.first = 1;
    P.src[1] = nullptr;  // the row id column is the position (k_rx_scatter4)
    P.src[2] = third;
    P.dst[0] = ws + Y.keys_a;
    P.dst[1] = with_rows ? ws + Y.rows_a : nullptr;
    P.dst[2] = third ? ws + Y.fp_a : nullptr;
    int rc = rx_pass(stream, P, Y.tiles1, (int64_t*)(ws + Y.cnt), (int64_t*)(ws + Y.scan), ws + Y.scan_ws, n, Y.bits2 ? seg1 : seg2);
    if (rc != HS_OK) return rc;
    T.keys = ws + Y.keys_a;
    T.rows = with_rows ? (const uint32_t*)(ws + Y.rows_a) : nullptr;
    if (third) T.third = (const uint32_t*)(ws + Y.fp_a);
    if (Y.bits2) {  // pass 2: the next bits2 bits inside every segment of pass 1
        P.seg_start = seg1;
        P.tile_base = (int64_t*)(ws + Y.tb1);
        P.n_seg = Y.nseg1;
        P.shift = low;
        P.bits = Y.bits2;
        P.first = 0;
        P.src[0] = ws + Y.keys_a;
        P.src[1] = with_rows ? ws + Y.rows_a : nullptr;
        P.src[2] = third ? ws + Y.fp_a : nullptr;
        P.dst[0] = ws + Y.keys_b;
        P.dst[1] = with_rows ? ws + Y.rows_b : nullptr;
        P.dst[2] = third ? ws + Y.fp_b : nullptr;
        rc = rx_pass(stream, P, Y.tiles2, (int64_t*)(ws + Y.cnt), (int64_t*)(ws + Y.scan), ws + Y.scan_ws, n, seg2);
        if (rc != HS_OK) return rc;
        T.keys = ws + Y.keys_b;
        T.rows = with_rows ? (const uint32_t*)(ws + Y.rows_b) : nullptr;
        if (third) T.third = (const uint32_t*)(ws + Y.fp_b);
    }
    return HS_OK;
}

// one launch path for the assembly kernels: one wave per partition, per_wave bytes of LDS each, wpb waves per block.  Each
// kernel whose blocks may take more than 64 KB of LDS (max_lds) asks for it once per device - every instantiation of this
// template has its own flag.
template <auto K, typename Args>
static int jx_assemble(hipStream_t stream, const char* who, const Args& A, int64_t parts, size_t per_wave, int wpb, int max_lds) {
    static unsigned long long attr_set = 0;
    if (max_lds > 65536 && hs_first_on_device(attr_set))
        (void)hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
    int64_t g = (parts + wpb - 1) / wpb;
    if (g > 256 * 32) g = 256 * 32;
    hipLaunchKernelGGL(K, dim3((unsigned)g), dim3(HS_WAVE * wpb), per_wave * wpb, stream, A);
    if (hipGetLastError() != hipSuccess) {
        hs_set_error("%s (assemble): kernel launch failed", who);
        return HS_E_LAUNCH;
    }
    return HS_OK;
}

extern "C" size_t hs_join_dense_ws_bytes(int64_t n_build, int64_t slots) {
    JxLayout Y;
    return jx_layout(JX_DENSE, n_build, slots, Y) ? Y.total : 0;
}

extern "C" int hs_join_dense_build(void* stream_, const int32_t* build_keys, int64_t n_build, int32_t key_min, int64_t slots,
                                   uint32_t* words, uint32_t* rows, uint32_t* list_count, void* ws_, uint32_t* flags) {
    JxLayout Y;
    if ((!build_keys && n_build > 0) || !words || !rows || !list_count || !ws_ || !flags || !jx_layout(JX_DENSE, n_build, slots, Y)) {
        hs_set_error("hs_join_dense_build: bad arguments (n_build < 2^31, 1 <= slots <= 2^29)");
        return HS_E_ARG;
    }
    hipStream_t stream = (hipStream_t)stream_;
    JxTuples T;
    const int rc = jx_partition(stream, "hs_join_dense_build", (uint8_t*)ws_, Y, n_build, build_keys, RX_BIN_RANGE, key_min, Y.L, nullptr, T);
    if (rc != HS_OK) return rc;
    const JdAssemble A{T.seg, T.parts, (const int32_t*)T.keys, T.rows, slots, key_min, Y.L, words, rows, list_count, n_build, flags};
    const size_t per_wave = (size_t)9 << Y.L;  // cursors + first rows (uint32) + tag bytes
    int wpb = (int)(65536 / per_wave);
    wpb = wpb < 1 ? 1 : (wpb > 4 ? 4 : wpb);
    return jx_assemble<k_jd_assemble>(stream, "hs_join_dense_build", A, T.parts, per_wave, wpb, 9 << JD_MAX_L);
}

struct JdProbe {
    const int32_t* keys;
    int64_t n, slots;
    int32_t key_min, pad;
    const uint32_t* words;
    const uint32_t* rows;
    const uint32_t* list_count;
    int64_t* counts;
    uint32_t* aux;  // [2 n]: first matching build row | start of the probe row's list in `rows`
    const int64_t* out_start;
    int64_t* out_left;
    int64_t* out_right;
};
typedef int jd_i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned jd_u32x4 __attribute__((ext_vector_type(4)));
typedef long long jd_i64x2 __attribute__((ext_vector_type(2)));

// a slot word -> the probe row's match count, first build row and list start (a list's length and first row are read only
// for a key with several partners)
__device__ __forceinline__ void jx_resolve(uint32_t word, const uint32_t* rows, const uint32_t* list_count, uint32_t& cnt, uint32_t& first,
                                           uint32_t& st) {
    const bool multi = word != JD_EMPTY && (word & JD_MULTI);
    st = multi ? word & ~JD_MULTI : 0u;
    cnt = word == JD_EMPTY ? 0u : 1u;
    first = word;
    if (multi) {
        cnt = list_count[st];
        first = rows[st];
    }
}

// the count pass's results for probe rows 4q .. 4q + 3 from their slot words: counts[], and in aux the first build rows,
// then (from `second` on) the list starts - 16-byte nontemporal stores where all four rows exist
__device__ __forceinline__ void jx_count_out(const uint32_t* word, int64_t q, int64_t n, const uint32_t* rows, const uint32_t* list_count,
                                             int64_t* counts, uint32_t* aux) {
    const int64_t second = (n + 3) & ~(int64_t)3;
    uint32_t cnt[4], first[4], st[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) jx_resolve(word[j], rows, list_count, cnt[j], first[j], st[j]);
    if (q * 4 + 3 < n) {
        int64_t* c = counts + q * 4;
        __builtin_nontemporal_store(jd_i64x2{(long long)cnt[0], (long long)cnt[1]}, reinterpret_cast<jd_i64x2*>(c));
        __builtin_nontemporal_store(jd_i64x2{(long long)cnt[2], (long long)cnt[3]}, reinterpret_cast<jd_i64x2*>(c + 2));
        __builtin_nontemporal_store(jd_u32x4{first[0], first[1], first[2], first[3]}, reinterpret_cast<jd_u32x4*>(aux) + q);
        __builtin_nontemporal_store(jd_u32x4{st[0], st[1], st[2], st[3]}, reinterpret_cast<jd_u32x4*>(aux + second) + q);
    } else {
        for (int j = 0; j < 4 && q * 4 + j < n; ++j) {
            counts[q * 4 + j] = (int64_t)cnt[j];
            aux[q * 4 + j] = first[j];
            aux[second + q * 4 + j] = st[j];
        }
    }
}

// Probe, pass 1: four keys per lane (one 16-byte load; buffers carry slack past n), ONE scattered 4-byte read per key - its
// slot word says "no partner", names the one partner, or points at a list (then, and only then, two more reads: the
// list's length and its first row); the four lookups of a lane are in flight together.  What the fill pass needs is written
// down sequentially (the first build row and the list's start: 8 bytes per probe row), so it never returns to the
// scattered arrays for a key with one partner - the usual case.
__global__ void __launch_bounds__(256) k_jd_count(const JdProbe A) {
    const int64_t nq = (A.n + 3) / 4;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) {
        const jd_i32x4 kv = __builtin_nontemporal_load(reinterpret_cast<const jd_i32x4*>(A.keys) + q);
        const int32_t k[4] = {kv.x, kv.y, kv.z, kv.w};
        uint32_t word[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t o = (int64_t)k[j] - (int64_t)A.key_min;
            const bool in = q * 4 + j < A.n && (uint64_t)o < (uint64_t)A.slots;
            word[j] = in ? A.words[o] : JD_EMPTY;
        }
        jx_count_out(word, q, A.n, A.rows, A.list_count, A.counts, A.aux);
    }
}


// Probe, pass 2: pairs ordered by probe row, then build row.  A stream: output offsets (their differences are the match
// counts), the first build rows, the pairs; only a probe row with several partners reads the rest of its list.
__global__ void __launch_bounds__(256) k_jd_fill(const JdProbe A) {
    const int64_t nq = (A.n + 3) / 4;
    const int64_t second = (A.n + 3) & ~(int64_t)3;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) {
        int64_t at[5];
        uint32_t first[4];
        if (q * 4 + 3 < A.n) {
            const jd_u32x4 f = __builtin_nontemporal_load(reinterpret_cast<const jd_u32x4*>(A.aux) + q);
            first[0] = f.x; first[1] = f.y; first[2] = f.z; first[3] = f.w;
#pragma unroll
            for (int j = 0; j < 5; ++j) at[j] = A.out_start[q * 4 + j];  // out_start has n + 1 entries
        } else {
            for (int j = 0; j < 5; ++j) at[j] = q * 4 + j <= A.n ? A.out_start[q * 4 + j] : A.out_start[A.n];
            for (int j = 0; j < 4; ++j) first[j] = q * 4 + j < A.n ? A.aux[q * 4 + j] : 0u;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t cnt = at[j + 1] - at[j];
            if (cnt <= 0) continue;
            const int64_t i = q * 4 + j;
            A.out_left[at[j]] = (int64_t)first[j];
            A.out_right[at[j]] = i;
            if (cnt > 1) {
                const uint32_t st = A.aux[second + i];
                for (int64_t r = 1; r < cnt; ++r) {
                    A.out_left[at[j] + r] = (int64_t)A.rows[st + r];
                    A.out_right[at[j] + r] = i;
                }
            }
        }
    }
}

static int jd_probe_args(const char* who, const int32_t* probe_keys, int64_t n_probe, int64_t slots, const uint32_t* words) {
    if ((!probe_keys && n_probe > 0) || !words || n_probe < 0 || slots < 1 || ((uintptr_t)probe_keys & 15)) {
        hs_set_error("%s: bad arguments (probe keys 16-byte aligned)", who);
        return HS_E_ARG;
    }
    return HS_OK;
}
extern "C" size_t hs_join_dense_aux_bytes(int64_t n_probe) { return n_probe < 0 ? 0 : (size_t)(((n_probe + 3) & ~(int64_t)3) * 2) * 4 + 64; }
extern "C" int hs_join_dense_count(void* stream, const int32_t* probe_keys, int64_t n_probe, int32_t key_min, int64_t slots,
                                   const uint32_t* words, const uint32_t* rows, const uint32_t* list_count, int64_t* counts, void* aux) {
    int rc = jd_probe_args("hs_join_dense_count", probe_keys, n_probe, slots, words);
    if (rc != HS_OK) return rc;
    if (!rows || !list_count || !counts || !aux || ((uintptr_t)counts & 15) || ((uintptr_t)aux & 15)) {
        hs_set_error("hs_join_dense_count: counts and aux must be 16-byte aligned");
        return HS_E_ARG;
    }
    if (n_probe == 0) return HS_OK;
    JdProbe A{probe_keys, n_probe, slots, key_min, 0, words, rows, list_count, counts, (uint32_t*)aux, nullptr, nullptr, nullptr};
    int64_t g = ((n_probe + 3) / 4 + 255) / 256;
    if (g > 256 * 64) g = 256 * 64;
    hipLaunchKernelGGL(k_jd_count, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, A);
    RX_CHECK_LAUNCH("hs_join_dense_count");
    return HS_OK;
}
extern "C" int hs_join_dense_fill(void* stream, int64_t n_probe, const uint32_t* rows, const void* aux, const int64_t* out_start,
                                  int64_t* out_left, int64_t* out_right) {
    if (n_probe < 0 || !rows || !aux || !out_start || !out_left || !out_right || ((uintptr_t)aux & 15)) {
        hs_set_error("hs_join_dense_fill: bad arguments");
        return HS_E_ARG;
    }
    if (n_probe == 0) return HS_OK;
    JdProbe A{nullptr, n_probe, 0, 0, 0, nullptr, rows, nullptr, nullptr, (uint32_t*)const_cast<void*>(aux), out_start, out_left, out_right};
    int64_t g = ((n_probe + 3) / 4 + 255) / 256;
    if (g > 256 * 64) g = 256 * 64;
    hipLaunchKernelGGL(k_jd_fill, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, A);
    RX_CHECK_LAUNCH("hs_join_dense_fill");
    return HS_OK;
}

// =====================================================================================================
// Key sets for LEFT SEMI / LEFT ANTI joins on INTEGER keys (include/hipspark.h hs_keyset_*)
// =====================================================================================================
// No reference counterpart: the reference runs every join kind as the inner join.  A semi join asks ONE BIT per key, so the
// build side becomes a bitmap over the key range - bit s of the bitmap = "some build key equals key_min + s" - and the probe
// one scattered 4-byte read per row.  The build follows the dense join's rule (move the rows, do not hammer global memory
// with scattered atomics) with half its traffic: the keys travel ALONE through the partition passes (jx_partition without
// rows), on the high bits of key - key_min, into partitions of 2^KS_L slots whose bits fit a workgroup's LDS; a key range of
// one partition takes no pass at all.  Work items are (partition, chunk of at most KS_CHUNK of its keys): clear the LDS bits,
// OR the chunk in (LDS atomics: order-free, all waves of the workgroup share the table), store the partition's words with
// coalesced 16-byte plain stores.  Only a partition too crowded for one chunk is zeroed up front (k_ks_plan) and merged
// with atomic ORs over its consecutive non-zero words - whole 256-byte lines per wave, never a scattered atomic.
constexpr int KS_L = 19;          // log2 of a partition's slots: 2^19 bits = 64 KB of LDS (measured: profiles/r25_semi_join.txt)
constexpr int KS_CHUNK = 65536;   // keys of one work item
constexpr int KS_THREADS = 1024;
constexpr int KS_SLACK = 64;      // bytes past the rounded words (zeroed by the build like every other word)

// tuning knobs of the measurement (tools/bench_semi_join.py): HIPSPARK_KEYSET_L = 16 .. 19, HIPSPARK_KEYSET_CHUNK = keys per work item
static int ks_partition_bits() {
    static const int L = [] {
        const char* e = getenv("HIPSPARK_KEYSET_L");
        const int v = e ? atoi(e) : KS_L;
        return v >= 32 - 2 * RX_MAX_BITS && v <= 19 ? v : KS_L;
    }();
    return L;
}
static int64_t ks_chunk_keys() {
    static const int64_t c = [] {
        const char* e = getenv("HIPSPARK_KEYSET_CHUNK");
        const long long v = e ? atoll(e) : (long long)KS_CHUNK;
        return (int64_t)(v >= 1024 && v <= ((long long)1 << 30) ? v : KS_CHUNK);
    }();
    return c;
}

struct KsBuild {
    const int64_t* seg;        // [parts + 1] key ranges of the partitions
    int64_t parts, last;       // last: the partition that holds slot `slots - 1` (partitions past it must be empty)
    const int32_t* keys;       // partitioned (the build column itself without a pass)
    int64_t slots, chunk;
    int32_t key_min, L;
    uint32_t* bitmap;
    int64_t words;             // all words of the buffer, slack included (a multiple of 4)
    int64_t* items;            // [parts] work items of every partition, then (item_start) their exclusive scan [parts + 1]
    const int64_t* item_start;
    uint32_t* flags;
};

// the words of partition p: [lo, hi) - the last live partition also owns the rounding and the slack behind it
__device__ __forceinline__ void ks_words(const KsBuild& A, int64_t p, int64_t& lo, int64_t& hi) {
    const int64_t pw = (int64_t)1 << (A.L - 5);
    lo = p * pw;
    hi = p == A.last ? A.words : lo + pw;
}

// work items per partition (a live one has at least one: its words are written even without a key); a partition of
// several chunks is zeroed here, ahead of the atomic merge
__global__ void __launch_bounds__(256) k_ks_plan(const KsBuild A) {
    for (int64_t p = blockIdx.x; p < A.parts; p += gridDim.x) {
        const int64_t len = A.seg[p + 1] - A.seg[p];
        const bool live = p <= A.last;
        if (threadIdx.x == 0) {
            A.items[p] = live ? (len > A.chunk ? (len + A.chunk - 1) / A.chunk : 1) : 0;
            if (!live && len > 0) atomicOr(A.flags, HS_FLAG_BAD_PROGRAM);  // a key past the declared range
        }
        if (live && len > A.chunk) {
            int64_t lo, hi;
            ks_words(A, p, lo, hi);
            jd_u32x4* out = reinterpret_cast<jd_u32x4*>(A.bitmap);
            for (int64_t q = lo / 4 + threadIdx.x; q < hi / 4; q += blockDim.x) out[q] = jd_u32x4{0u, 0u, 0u, 0u};
        }
    }
}

__global__ void __launch_bounds__(KS_THREADS) k_ks_build(const KsBuild A) {
    extern __shared__ __align__(16) uint32_t ks_bits[];  // 2^(L - 5) words
    const int tid = threadIdx.x;
    const int64_t pw = (int64_t)1 << (A.L - 5);
    const uint32_t kmin = (uint32_t)A.key_min, smask = (1u << A.L) - 1u;
    const int64_t n_items = A.item_start[A.parts];
    uint32_t err = 0;
    for (int64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        int64_t lo_p = 0, hi_p = A.parts;  // the last p with item_start[p] <= item owns it (dead partitions share the total)
        while (hi_p - lo_p > 1) {
            const int64_t mid = (lo_p + hi_p) >> 1;
            if (A.item_start[mid] <= item) lo_p = mid;
            else hi_p = mid;
        }
        const int64_t p = lo_p, c = item - A.item_start[p], chunks = A.item_start[p + 1] - A.item_start[p];
        const int64_t b = A.seg[p] + c * A.chunk;
        const int64_t e = b + A.chunk < A.seg[p + 1] ? b + A.chunk : A.seg[p + 1];
        for (int64_t q = tid; q < pw / 4; q += KS_THREADS) reinterpret_cast<jd_u32x4*>(ks_bits)[q] = jd_u32x4{0u, 0u, 0u, 0u};
        __syncthreads();
        for (int64_t base = b; base < e; base += (int64_t)KS_THREADS * 4) {
            uint32_t s[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {  // four coalesced loads in flight; slot = key - key_min as uint32 (k_jd_count's rule)
                const int64_t i = base + (int64_t)j * KS_THREADS + tid;
                s[j] = i < e ? (uint32_t)A.keys[i] - kmin : 0u;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (base + (int64_t)j * KS_THREADS + tid >= e) continue;
                if ((int64_t)s[j] < A.slots && (int64_t)(s[j] >> A.L) == p) atomicOr(&ks_bits[(s[j] & smask) >> 5], 1u << (s[j] & 31u));
                else err = HS_FLAG_BAD_PROGRAM;  // outside the declared range (or the partition): no bit is set
            }
        }
        __syncthreads();
        int64_t lo, hi;
        ks_words(A, p, lo, hi);
        if (chunks == 1) {
            for (int64_t q = tid; q < (hi - lo) / 4; q += KS_THREADS) {
                const jd_u32x4 v = q < pw / 4 ? reinterpret_cast<const jd_u32x4*>(ks_bits)[q] : jd_u32x4{0u, 0u, 0u, 0u};
                reinterpret_cast<jd_u32x4*>(A.bitmap + lo)[q] = v;
            }
        } else {  // (k_ks_plan zeroed [lo, hi)) consecutive lanes, consecutive words: a wave's atomics fall into whole lines
            for (int64_t w = tid; w < pw; w += KS_THREADS) {
                const uint32_t v = ks_bits[w];
                if (v) atomicOr(A.bitmap + lo + w, v);
            }
        }
        __syncthreads();  // the table is cleared again for the next item
    }
    if (err) atomicOr(A.flags, err);
}

static int64_t ks_words_total(int64_t slots) { return (((slots + 31) / 32 + 3) & ~(int64_t)3) + KS_SLACK / 4; }

struct KsLayout {
    JxLayout Y;
    size_t items, item_start, scan_ws, total;
};
static bool ks_layout(int64_t n, int64_t slots, KsLayout& K) {
    K.Y.L = ks_partition_bits();
    if (!jx_layout(JX_KEYSET, n, slots, K.Y)) return false;
    size_t off = K.Y.total;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += rx_align(bytes);
        return at;
    };
    K.items = take((size_t)K.Y.parts * 8);
    K.item_start = take((size_t)(K.Y.parts + 1) * 8);
    K.scan_ws = take(hs_scan_ws_bytes(K.Y.parts));
    K.total = off;
    return true;
}

extern "C" size_t hs_keyset_bitmap_bytes(int64_t slots) {
    return slots < 1 || slots > ((int64_t)1 << 32) ? 0 : (size_t)ks_words_total(slots) * 4;
}
extern "C" size_t hs_keyset_ws_bytes(int64_t n_build, int64_t slots) {
    KsLayout K;
    return ks_layout(n_build, slots, K) ? K.total : 0;
}

extern "C" int hs_keyset_build(void* stream_, const int32_t* keys, int64_t n, int32_t key_min, int64_t slots, uint32_t* bitmap,
                               void* ws_, uint32_t* flags) {
    KsLayout K;
    if ((!keys && n > 0) || !bitmap || !ws_ || !flags || ((uintptr_t)bitmap & 15) || !ks_layout(n, slots, K) ||
        (int64_t)key_min + slots - 1 > 0x7fffffffll) {
        hs_set_error("hs_keyset_build: bad arguments (n < 2^31, 1 <= slots <= 2^32, key_min + slots - 1 an int32, bitmap 16-byte aligned)");
        return HS_E_ARG;
    }
    hipStream_t stream = (hipStream_t)stream_;
    uint8_t* ws = (uint8_t*)ws_;
    const JxLayout& Y = K.Y;
    JxTuples T;
    int rc = jx_partition(stream, "hs_keyset_build", ws, Y, n, keys, RX_BIN_RANGE, key_min, Y.L, nullptr, T, false);
    if (rc != HS_OK) return rc;
    const KsBuild A{T.seg, T.parts, (slots - 1) >> Y.L, (const int32_t*)T.keys, slots, ks_chunk_keys(), key_min, Y.L, bitmap,
                    ks_words_total(slots), (int64_t*)(ws + K.items), (const int64_t*)(ws + K.item_start), flags};
    hipLaunchKernelGGL(k_ks_plan, dim3((unsigned)(T.parts < 4096 ? T.parts : 4096)), dim3(256), 0, stream, A);
    RX_CHECK_LAUNCH("hs_keyset_build (plan)");
    rc = hs_exclusive_scan_i64(stream, A.items, T.parts, (int64_t*)(ws + K.item_start), ws + K.scan_ws);
    if (rc != HS_OK) return rc;
    const size_t lds = (size_t)4 << (Y.L - 5);
    static unsigned long long attr_set = 0;
    if (hs_first_on_device(attr_set))
        (void)hipFuncSetAttribute((const void*)k_ks_build, hipFuncAttributeMaxDynamicSharedMemorySize, 4 << (19 - 5));
    int64_t g = A.last + 1 + n / A.chunk;  // >= the work items: one per live partition and one per further whole chunk
    if (g > 256 * 8) g = 256 * 8;
    hipLaunchKernelGGL(k_ks_build, dim3((unsigned)g), dim3(KS_THREADS), lds, stream, A);
    RX_CHECK_LAUNCH("hs_keyset_build");
    return HS_OK;
}

struct KsProbe {
    const int32_t* keys;
    int64_t n, slots;
    int32_t key_min, anti;
    const uint32_t* bitmap;
    uint8_t* mask;
};
// Probe (modelled on k_jd_count): four keys per lane from one 16-byte non-temporal load, their four word reads in flight
// together, a key outside [key_min, key_min + slots) is a non-member without a read; one byte per row leaves as a packed
// 4-byte store.  The last, partial quad reads and writes its rows one by one: nothing past n is touched.
__global__ void __launch_bounds__(256) k_ks_probe(const KsProbe A) {
    const int64_t nq = (A.n + 3) / 4;
    const uint32_t flip = A.anti ? 1u : 0u;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) {
        const bool whole = q * 4 + 3 < A.n;
        int32_t k[4] = {0, 0, 0, 0};
        if (whole) {
            const jd_i32x4 kv = __builtin_nontemporal_load(reinterpret_cast<const jd_i32x4*>(A.keys) + q);
            k[0] = kv.x; k[1] = kv.y; k[2] = kv.z; k[3] = kv.w;
        } else {
            for (int j = 0; j < 4 && q * 4 + j < A.n; ++j) k[j] = A.keys[q * 4 + j];
        }
        uint32_t word[4], bit[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t o = (int64_t)k[j] - (int64_t)A.key_min;
            const bool in = q * 4 + j < A.n && (uint64_t)o < (uint64_t)A.slots;
            word[j] = in ? A.bitmap[o >> 5] : 0u;
            bit[j] = (uint32_t)o & 31u;
        }
        uint32_t packed = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) packed |= (((word[j] >> bit[j]) & 1u) ^ flip) << (8 * j);
        if (whole) __builtin_nontemporal_store(packed, reinterpret_cast<uint32_t*>(A.mask) + q);
        else
            for (int j = 0; j < 4 && q * 4 + j < A.n; ++j) A.mask[q * 4 + j] = (uint8_t)(packed >> (8 * j));
    }
}

extern "C" int hs_keyset_probe(void* stream, const int32_t* keys, int64_t n, int32_t key_min, int64_t slots, const uint32_t* bitmap,
                               int32_t anti, uint8_t* mask) {
    if ((!keys && n > 0) || !bitmap || (!mask && n > 0) || n < 0 || n >= 0x7fffffffll || slots < 1 || slots > ((int64_t)1 << 32) ||
        ((uintptr_t)keys & 15) || ((uintptr_t)mask & 3)) {
        hs_set_error("hs_keyset_probe: bad arguments (n < 2^31, 1 <= slots <= 2^32, probe keys 16-byte aligned, mask 4-byte aligned)");
        return HS_E_ARG;
    }
    if (n == 0) return HS_OK;
    const KsProbe A{keys, n, slots, key_min, anti ? 1 : 0, bitmap, mask};
    int64_t g = ((n + 3) / 4 + 255) / 256;
    if (g > 256 * 64) g = 256 * 64;
    hipLaunchKernelGGL(k_ks_probe, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, A);
    RX_CHECK_LAUNCH("hs_keyset_probe");
    return HS_OK;
}

// the count pass of the hashed / global-table joins as the same mask: (counts[i] != 0) != anti
__global__ void __launch_bounds__(256) k_mask_from_counts(const int64_t* counts, int64_t n, uint32_t flip, uint8_t* mask) {
    const int64_t nq = (n + 3) / 4;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) {
        if (q * 4 + 3 < n) {
            const jd_i64x2 a = __builtin_nontemporal_load(reinterpret_cast<const jd_i64x2*>(counts) + 2 * q);
            const jd_i64x2 b = __builtin_nontemporal_load(reinterpret_cast<const jd_i64x2*>(counts) + 2 * q + 1);
            const uint32_t packed = ((a.x != 0 ? 1u : 0u) ^ flip) | (((a.y != 0 ? 1u : 0u) ^ flip) << 8) |
                                    (((b.x != 0 ? 1u : 0u) ^ flip) << 16) | (((b.y != 0 ? 1u : 0u) ^ flip) << 24);
            __builtin_nontemporal_store(packed, reinterpret_cast<uint32_t*>(mask) + q);
        } else {
            for (int j = 0; j < 4 && q * 4 + j < n; ++j) mask[q * 4 + j] = (uint8_t)((counts[q * 4 + j] != 0 ? 1u : 0u) ^ flip);
        }
    }
}

extern "C" int hs_mask_from_counts(void* stream, const int64_t* counts, int64_t n, int32_t anti, uint8_t* mask) {
    if (n < 0 || ((!counts || !mask) && n > 0) || ((uintptr_t)counts & 15) || ((uintptr_t)mask & 3)) {
        hs_set_error("hs_mask_from_counts: bad arguments (counts 16-byte aligned, mask 4-byte aligned)");
        return HS_E_ARG;
    }
    if (n == 0) return HS_OK;
    int64_t g = ((n + 3) / 4 + 255) / 256;
    if (g > 256 * 64) g = 256 * 64;
    hipLaunchKernelGGL(k_mask_from_counts, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, counts, n, anti ? 1u : 0u, mask);
    RX_CHECK_LAUNCH("hs_mask_from_counts");
    return HS_OK;
}

// =====================================================================================================
// The general inner join on ANY INTEGER keys (round 4; include/hipspark.h hs_join_hash_*)
// =====================================================================================================
// Same reference loop as above (tasks.py:201-240), for keys the dense form does not hold: a sparse or huge key range,
// negative keys, a few hot values.  The table is an open-addressing table of 8-byte slots {key, word} cut into WINDOWS of
// 2^JH_L slots; a key belongs to window jh_window(key) and probes linearly INSIDE it (wrapping at the window's end), so
//   * the build never leaves LDS: the (key, row) tuples are brought into window order by the two stable partition passes
//     (RX_BIN_WINDOW), one wave per window inserts its keys into an LDS copy of the window (ds_cmpst on a 64-bit cell),
//     counts, scans and places the rows in order exactly like the dense form, and stores the finished window with coalesced
//     8-byte stores - no global atomic, no scattered store, every list ascending without a sort;
//   * a probe is ONE scattered 8-byte read in the usual case (the slot holds key and word together; at a load of ~0.57 a
//     present key sits 1.7 slots from its start on average - the same 64-byte line nearly always).
// The slot word is the dense form's (JD_EMPTY / the one build row / JD_MULTI + list start), rows[] and list_count[] too, so
// the probe's second pass IS hs_join_dense_fill.
// slots per window, log2 (JH_L_SMALL / JH_L_LARGE): 512 (8.5 KB of LDS per wave: key cells, cursors, first rows, tag bytes
// - 18 waves per CU) while 65 536 windows hold the build side (19 M rows), else 1024 (17 KB: 9 waves per CU; 38 M rows).
// The assembly is a chain of LDS round trips per 64-tuple step, one wave per window: it runs on the number of waves a CU
// holds.
constexpr uint64_t JH_FREE = ~0ull;            // LDS key cell: nobody here yet (a key occupies the low 32 bits only)

struct JhAssemble {
    const int64_t* seg_start;  // [parts + 1] tuple ranges of the partitions = windows (parts >= windows; the rest are empty)
    int64_t parts, windows;
    const uint32_t* keys;      // tuples, window by window, in row order inside a window: the INTEGER keys | the STRING fingerprints
    const uint32_t* rows;
    hs_col key;                // STRING: the build key column (byte compares)
    uint2* table;              // [windows << L] {key | fingerprint, word}
    uint32_t* out_rows;        // [n]: build rows window by window, slot by slot, ascending within a slot
    uint32_t* list_count;      // [n]: at the start of a list of several rows, its length
    uint16_t* slot_of;         // [n] scratch: the slot every tuple found in the counting pass (the placement pass reads it back
                               // with coalesced loads instead of walking the LDS window again)
    uint32_t* status;          // HS_FLAG_DICT_FULL only
    uint32_t* flags;           // anything else
};

// slot of `key` in the wave's LDS window, claiming a free cell on the way when INSERT; -1: the window is full (more
// distinct keys than slots - jh_windows leaves 1.75x room over the AVERAGE window; the caller falls back)
template <bool INSERT, int JH_L>
__device__ __forceinline__ int jh_slot(uint64_t* cell, uint32_t key, uint32_t start) {
    constexpr uint32_t wmask = (1u << JH_L) - 1u;
    uint32_t s = start & wmask;
    for (int probe = 0; probe <= (int)wmask; ++probe) {
        uint64_t cur = __hip_atomic_load(&cell[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (INSERT && cur == JH_FREE) {
            cur = atomicCAS((unsigned long long*)&cell[s], (unsigned long long)JH_FREE, (unsigned long long)key);
            if (cur == JH_FREE) return (int)s;
        }
        if (cur == (uint64_t)key) return (int)s;
        if (!INSERT && cur == JH_FREE) return -1;
        s = (s + 1) & wmask;
    }
    return -1;
}

template <int JH_L>
__device__ __forceinline__ int js_slot(uint64_t* cell, const hs_col& key, uint32_t fp, uint32_t row);  // (the STRING section)

// One wave per window of 2^JH_L slots: its tuples claim LDS key cells, then counts, scan, ordered placement and the finished
// window (jx_*).  The key form is the only difference: an INTEGER tuple claims its key's cell (jh_slot), a STRING tuple
// (fingerprint, row) a cell of its fingerprint whose key bytes are its own (js_slot).  A window with more distinct keys than
// slots is stored empty and raises HS_FLAG_DICT_FULL in *status.
template <int JH_L, bool STR>
__global__ void __launch_bounds__(256) k_jh_assemble(const JhAssemble A) {
    extern __shared__ __align__(16) uint64_t jh_lds[];
    constexpr int W = 1 << JH_L;
    const int lane = threadIdx.x & (HS_WAVE - 1), w = threadIdx.x / HS_WAVE, wpb = blockDim.x / HS_WAVE;
    uint64_t* cell = jh_lds + (size_t)w * (2 * W + W / 8);   // key cells
    uint32_t* cur = (uint32_t*)(cell + W);
    uint32_t* head = cur + W;
    uint8_t* tag = (uint8_t*)(head + W);
    const auto tuple_at = [&](int64_t i) { return make_uint2(A.keys[i], STR ? A.rows[i] : 0u); };
    const auto claim = [&](uint2 t, int64_t i) {
        const int s = STR ? js_slot<JH_L>(cell, A.key, t.x, t.y) : jh_slot<true, JH_L>(cell, t.x, rx_mix32(t.x));
        A.slot_of[i] = (uint16_t)s;
        return s;
    };
    uint32_t err = 0, full_any = 0;
    for (int64_t p = (int64_t)blockIdx.x * wpb + w; p < A.parts; p += (int64_t)gridDim.x * wpb) {
        const int64_t b = A.seg_start[p], e = A.seg_start[p + 1];
        if (p >= A.windows) {
            if (e > b) err |= HS_FLAG_BAD_PROGRAM;  // a tuple past the last window: the passes and the table disagree
            continue;
        }
        const bool full = jx_count(cur, head, JH_L, b, e, lane, tuple_at, [&](int s) { cell[s] = JH_FREE; }, claim);
        if (__ballot(full)) {  // (wave-uniform) leave the window empty and say so
            full_any = HS_FLAG_DICT_FULL;
            for (int s = lane; s < W; s += HS_WAVE) A.table[(p << JH_L) + s] = make_uint2(0u, JD_EMPTY);
            continue;
        }
        jx_scan(cur, JH_L, lane);
        jx_place(cur, head, tag, JH_L, b, e, lane, [&](int64_t i) { return (uint32_t)A.slot_of[i]; }, [](uint32_t s) { return s; }, A.rows,
                 A.out_rows);
        jx_emit(cur, head, b, W, lane, A.list_count,
                [&](int s, uint32_t word) { A.table[(p << JH_L) + s] = make_uint2((uint32_t)cell[s], word); });
    }
    if (full_any && lane == 0) atomicOr(A.status, full_any);
    if (err && lane == 0) atomicOr(A.flags, err);
}

// the assembly of the hashed forms over the partitioned tuples T (the window number's passes)
template <bool STR>
static int jh_assemble(hipStream_t stream, const char* who, const JxLayout& Y, const JxTuples& T, const hs_col& key, uint8_t* ws, void* table,
                       uint32_t* rows, uint32_t* list_count, uint32_t* status, uint32_t* flags) {
    const JhAssemble A{T.seg, T.parts, Y.windows, STR ? T.third : (const uint32_t*)T.keys, T.rows, key, (uint2*)table, rows, list_count,
                       (uint16_t*)(ws + Y.slot_of), status, flags};
    const size_t per_wave = (size_t)17 << Y.L;  // key cells (8 B) + cursors + first rows (4 B each) + tag bytes
    constexpr int wpb = 4;
    if (Y.L == JH_L_SMALL) return jx_assemble<k_jh_assemble<JH_L_SMALL, STR>>(stream, who, A, T.parts, per_wave, wpb, (17 << JH_L_SMALL) * wpb);
    return jx_assemble<k_jh_assemble<JH_L_LARGE, STR>>(stream, who, A, T.parts, per_wave, wpb, (17 << JH_L_LARGE) * wpb);
}

extern "C" size_t hs_join_hash_ws_bytes(int64_t n_build) {
    JxLayout Y;
    return jx_layout(JX_HASH, n_build, 0, Y) ? Y.total : 0;
}
extern "C" int64_t hs_join_hash_slots(int64_t n_build) {
    JxLayout Y;
    return jx_layout(JX_HASH, n_build, 0, Y) ? Y.windows << Y.L : 0;
}

extern "C" int hs_join_hash_build(void* stream_, const int32_t* build_keys, int64_t n_build, void* table, uint32_t* rows,
                                  uint32_t* list_count, void* ws_, uint32_t* status, uint32_t* flags) {
    JxLayout Y;
    if ((!build_keys && n_build > 0) || !table || !rows || !list_count || !ws_ || !status || !flags || ((uintptr_t)table & 7) ||
        !jx_layout(JX_HASH, n_build, 0, Y)) {
        hs_set_error("hs_join_hash_build: bad arguments (n_build <= 38 M rows, table 8-byte aligned)");
        return HS_E_ARG;
    }
    hipStream_t stream = (hipStream_t)stream_;
    uint8_t* ws = (uint8_t*)ws_;
    JxTuples T;
    const int rc = jx_partition(stream, "hs_join_hash_build", ws, Y, n_build, build_keys, RX_BIN_WINDOW, (int32_t)Y.windows, 0, nullptr, T);
    if (rc != HS_OK) return rc;
    return jh_assemble<false>(stream, "hs_join_hash_build", Y, T, hs_col{}, ws, table, rows, list_count, status, flags);
}

struct JhProbe {
    const int32_t* keys;
    int64_t n;
    uint32_t windows, pad;
    const uint2* table;
    const uint32_t* rows;
    const uint32_t* list_count;
    int64_t* counts;
    uint32_t* aux;
};

// Probe, pass 1 (the hashed twin of k_jd_count): four keys per lane, their first slots in flight together; a slot that
// holds another key sends the lane to the next one of the window.  counts / aux as hs_join_dense_count writes them.
template <int JH_L>
__global__ void __launch_bounds__(256) k_jh_count(const JhProbe A) {
    constexpr uint32_t wmask = (1u << JH_L) - 1u;
    const int64_t nq = (A.n + 3) / 4;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) {
        const jd_i32x4 kv = __builtin_nontemporal_load(reinterpret_cast<const jd_i32x4*>(A.keys) + q);
        const uint32_t k[4] = {(uint32_t)kv.x, (uint32_t)kv.y, (uint32_t)kv.z, (uint32_t)kv.w};
        uint32_t word[4], at[4];
        const uint2* win[4];
        uint2 slot[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t h = rx_mix32(k[j]);
            win[j] = A.table + ((int64_t)(((uint64_t)h * A.windows) >> 32) << JH_L);
            at[j] = h & wmask;
            slot[j] = win[j][at[j]];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            for (int probe = 0; probe < (int)wmask && slot[j].y != JD_EMPTY && slot[j].x != k[j]; ++probe) {
                at[j] = (at[j] + 1) & wmask;
                slot[j] = win[j][at[j]];
            }
            word[j] = q * 4 + j < A.n && slot[j].x == k[j] ? slot[j].y : JD_EMPTY;
        }
        jx_count_out(word, q, A.n, A.rows, A.list_count, A.counts, A.aux);
    }
}

extern "C" int hs_join_hash_count(void* stream, const int32_t* probe_keys, int64_t n_probe, int64_t n_build, const void* table,
                                  const uint32_t* rows, const uint32_t* list_count, int64_t* counts, void* aux) {
    JxLayout Y;
    if ((!probe_keys && n_probe > 0) || n_probe < 0 || !table || !rows || !list_count || !counts || !aux || ((uintptr_t)probe_keys & 15) ||
        ((uintptr_t)counts & 15) || ((uintptr_t)aux & 15) || !jx_layout(JX_HASH, n_build, 0, Y)) {
        hs_set_error("hs_join_hash_count: bad arguments (probe keys, counts and aux 16-byte aligned; n_build as given to the build)");
        return HS_E_ARG;
    }
    if (n_probe == 0) return HS_OK;
    JhProbe A{probe_keys, n_probe, (uint32_t)Y.windows, 0, (const uint2*)table, rows, list_count, counts, (uint32_t*)aux};
    int64_t g = ((n_probe + 3) / 4 + 255) / 256;
    if (g > 256 * 64) g = 256 * 64;
    if (Y.L == JH_L_SMALL) hipLaunchKernelGGL(k_jh_count<JH_L_SMALL>, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, A);
    else hipLaunchKernelGGL(k_jh_count<JH_L_LARGE>, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, A);
    RX_CHECK_LAUNCH("hs_join_hash_count");
    return HS_OK;
}

// =====================================================================================================
// The general inner join on STRING keys (round 5; include/hipspark.h hs_join_hash_str_*)
// =====================================================================================================
// The hashed form above for keys of any byte length.  A key's 64-bit FNV-1a h (hs_fnv1a, the hash the shuffle already uses
// for strings) goes through the 64-bit finaliser hs_mix64 - FNV-1a's high bits barely depend on the last bytes of a short
// key (a multiply only carries upwards: keys that differ in their trailing digits crowded a few windows and overflowed
// them) - and m = hs_mix64(h) is cut in two: the high 32 bits pick the WINDOW (multiply-shift, (m >> 32) * windows >> 32),
// the low 32 bits are the FINGERPRINT stored in the slot, and fp & (2^L - 1) is the slot where the key starts probing.
// Slots are {fingerprint, word}, the word as in the dense and hashed forms, so the probe is one scattered 8-byte read in the
// usual case.  A fingerprint never decides a match on its own: the probe compares the key's bytes with the first build row
// of the slot's list, the build compares bytes with the slot's representative row whenever a fingerprint is met again (a
// duplicate key, or - rarely - another key of the same fingerprint in the same window, which then takes its own slot).
// Build: one pass hashes every key (window number, fingerprint), two stable partition passes (RX_BIN_RANGE on the
// window number) bring the (window, row, fingerprint) tuples into window order, and one wave per window inserts, counts,
// scans and places them in LDS: k_jh_assemble<L, true>.  Geometry (windows, L, workspace arrays) is jx_layout's.
__device__ __forceinline__ uint32_t js_window(uint64_t m, uint32_t windows) { return (uint32_t)(((m >> 32) * (uint64_t)windows) >> 32); }

// hs_mix64(hs_fnv1a(key)), from at most three aligned word loads when the key is <= 16 bytes long
__device__ __forceinline__ uint64_t js_hash(const HsStr s) {
    if (s.len > 16) return hs_mix64(hs_fnv1a(s.p, s.len));
    uint64_t w0, w1;
    hs_str_words16(s.p, s.len, w0, w1);
    uint64_t h = 0xcbf29ce484222325ull;
    for (uint32_t i = 0; i < s.len; ++i) {
        h ^= ((i < 8 ? w0 >> (8 * i) : w1 >> (8 * (i - 8))) & 0xffu);
        h *= 0x100000001b3ull;
    }
    return hs_mix64(h);
}

__device__ __forceinline__ bool js_equal(const HsStr a, const HsStr b) {
    if (a.len != b.len) return false;
    if (a.len <= 16) {
        uint64_t a0, a1, b0, b1;
        hs_str_words16(a.p, a.len, a0, a1);
        hs_str_words16(b.p, b.len, b0, b1);
        return a0 == b0 && a1 == b1;
    }
    for (uint32_t i = 0; i < a.len; ++i)
        if (a.p[i] != b.p[i]) return false;
    return true;
}

__global__ void __launch_bounds__(256) k_js_hash(const hs_col key, int64_t n, uint32_t windows, uint32_t* win, uint32_t* fp) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t h = js_hash(hs_str_at(key, i));
        win[i] = js_window(h, windows);
        fp[i] = (uint32_t)h;
    }
}

// slot of the key of build row `row` (fingerprint fp) in the wave's LDS window, claiming a free cell when it meets one first;
// -1: the window is full
template <int JH_L>
__device__ __forceinline__ int js_slot(uint64_t* cell, const hs_col& key, uint32_t fp, uint32_t row) {
    constexpr uint32_t wmask = (1u << JH_L) - 1u;
    const uint64_t mine = (uint64_t)fp | ((uint64_t)row << 32);
    const HsStr k = hs_str_at(key, row);
    uint32_t s = fp & wmask;
    for (int probe = 0; probe <= (int)wmask; ++probe) {
        uint64_t cur = __hip_atomic_load(&cell[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (cur == JH_FREE) {
            cur = atomicCAS((unsigned long long*)&cell[s], (unsigned long long)JH_FREE, (unsigned long long)mine);
            if (cur == JH_FREE) return (int)s;
        }
        if ((uint32_t)cur == fp && js_equal(k, hs_str_at(key, (int64_t)(cur >> 32)))) return (int)s;
        s = (s + 1) & wmask;
    }
    return -1;
}

extern "C" size_t hs_join_hash_str_ws_bytes(int64_t n_build) {
    JxLayout Y;
    return jx_layout(JX_HASH_STR, n_build, 0, Y) ? Y.total : 0;
}
extern "C" int64_t hs_join_hash_str_slots(int64_t n_build) {
    JxLayout Y;
    return jx_layout(JX_HASH_STR, n_build, 0, Y) ? Y.windows << Y.L : 0;
}

static bool js_str_col(const hs_col* c) { return c && c->kind == HS_STR && (c->fixed_len >= 0 || (c->lens && c->offs)); }

extern "C" int hs_join_hash_str_build(void* stream_, const hs_col* build_key, int64_t n_build, void* table, uint32_t* rows,
                                      uint32_t* list_count, void* ws_, uint32_t* status, uint32_t* flags) {
    JxLayout Y;
    if ((n_build > 0 && !js_str_col(build_key)) || !build_key || !table || !rows || !list_count || !ws_ || !status || !flags ||
        ((uintptr_t)table & 7) || !jx_layout(JX_HASH_STR, n_build, 0, Y)) {
        hs_set_error("hs_join_hash_str_build: bad arguments (a STRING key column, n_build <= 38 M rows, table 8-byte aligned)");
        return HS_E_ARG;
    }
    hipStream_t stream = (hipStream_t)stream_;
    uint8_t* ws = (uint8_t*)ws_;
    const int64_t n = n_build;
    uint32_t* win = (uint32_t*)(ws + Y.win);
    uint32_t* fp = (uint32_t*)(ws + Y.fp);
    if (n > 0) {
        int64_t g = (n + 255) / 256;
        g = g > 4096 ? 4096 : g;
        hipLaunchKernelGGL(k_js_hash, dim3((unsigned)g), dim3(256), 0, stream, *build_key, n, (uint32_t)Y.windows, win, fp);
        RX_CHECK_LAUNCH("hs_join_hash_str_build (hash)");
    }
    // the partition key is the window number itself (RX_BIN_RANGE, no bias); the fingerprint travels along
    JxTuples T;
    const int rc = jx_partition(stream, "hs_join_hash_str_build", ws, Y, n, win, RX_BIN_RANGE, 0, 0, fp, T);
    if (rc != HS_OK) return rc;
    return jh_assemble<true>(stream, "hs_join_hash_str_build", Y, T, *build_key, ws, table, rows, list_count, status, flags);
}

struct JsProbe {
    hs_col build, probe;
    int64_t n;
    uint32_t windows, pad;
    const uint2* table;
    const uint32_t* rows;
    const uint32_t* list_count;
    int64_t* counts;
    uint32_t* aux;
};

// Probe, pass 1: one probe row per lane - hash, one 8-byte slot read, and on a fingerprint match one compare with the
// list's first build row (length, then bytes); a mismatch keeps probing inside the window.  counts / aux as
// hs_join_dense_count writes them.
template <int JH_L>
__global__ void __launch_bounds__(256) k_js_count(const JsProbe A) {
    constexpr uint32_t wmask = (1u << JH_L) - 1u;
    const int64_t second = (A.n + 3) & ~(int64_t)3;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < A.n; i += (int64_t)gridDim.x * blockDim.x) {
        const HsStr k = hs_str_at(A.probe, i);
        const uint64_t h = js_hash(k);
        const uint32_t fp = (uint32_t)h;
        const uint2* win = A.table + ((int64_t)js_window(h, A.windows) << JH_L);
        uint32_t at = fp & wmask;
        uint32_t word = JD_EMPTY, first = JD_EMPTY, st = 0u;
        uint2 slot = win[at];
        for (int probe = 0; probe <= (int)wmask && slot.y != JD_EMPTY; ++probe) {
            if (slot.x == fp) {
                const bool multi = (slot.y & JD_MULTI) != 0u;
                const uint32_t f = multi ? A.rows[slot.y & ~JD_MULTI] : slot.y;
                if (js_equal(k, hs_str_at(A.build, f))) {
                    word = slot.y;
                    first = f;
                    st = multi ? slot.y & ~JD_MULTI : 0u;
                    break;
                }
            }
            at = (at + 1) & wmask;
            slot = win[at];
        }
        const uint32_t cnt = word == JD_EMPTY ? 0u : (word & JD_MULTI) ? A.list_count[st] : 1u;
        A.counts[i] = (int64_t)cnt;
        A.aux[i] = first;
        A.aux[second + i] = st;
    }
}

extern "C" int hs_join_hash_str_count(void* stream, const hs_col* build_key, const hs_col* probe_key, int64_t n_probe, int64_t n_build,
                                      const void* table, const uint32_t* rows, const uint32_t* list_count, int64_t* counts, void* aux) {
    JxLayout Y;
    if (n_probe < 0 || !build_key || !probe_key || (n_probe > 0 && !js_str_col(probe_key)) || (n_build > 0 && !js_str_col(build_key)) ||
        !table || !rows || !list_count || !counts || !aux || ((uintptr_t)counts & 15) || ((uintptr_t)aux & 15) || !jx_layout(JX_HASH_STR, n_build, 0, Y)) {
        hs_set_error("hs_join_hash_str_count: bad arguments (STRING key columns, counts and aux 16-byte aligned; n_build as given to the build)");
        return HS_E_ARG;
    }
    if (n_probe == 0) return HS_OK;
    JsProbe A{*build_key, *probe_key, n_probe, (uint32_t)Y.windows, 0, (const uint2*)table, rows, list_count, counts, (uint32_t*)aux};
    int64_t g = (n_probe + 255) / 256;
    if (g > 256 * 64) g = 256 * 64;
    if (Y.L == JH_L_SMALL) hipLaunchKernelGGL(k_js_count<JH_L_SMALL>, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, A);
    else hipLaunchKernelGGL(k_js_count<JH_L_LARGE>, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, A);
    RX_CHECK_LAUNCH("hs_join_hash_str_count");
    return HS_OK;
}

// =====================================================================================================
// The general inner join: one route planner and one table handle (include/hipspark.h hs_join_table_*)
// =====================================================================================================
// Host code only.  hs_join_table_plan owns the routing rule of the four forms and the layout of the form's arrays inside one
// allocation; build / count / fill hand the planned parts to the form's own entry points.  A caller's fallback ladder is
// "plan again without the route whose window overflowed".
namespace {
struct JtParts {
    uint8_t* p[4];
    JtParts(const hs_join_table& t, const void* table) {
        for (int i = 0; i < 4; ++i) p[i] = (uint8_t*)const_cast<void*>(table) + t.part[i];
    }
    template <class T>
    T* at(int i) const { return (T*)p[i]; }
};

bool jt_args(const char* who, const hs_join_table* t, const hs_col* build_key, const hs_col* probe_key, const void* table) {
    if (t && build_key && probe_key && table && t->route >= HS_JOIN_ROUTE_DENSE && t->route <= HS_JOIN_ROUTE_GLOBAL) return true;
    hs_set_error("%s: bad arguments (a planned table with a route)", who);
    return false;
}
}  // namespace

extern "C" int hs_join_table_plan(const hs_col* build_key, const hs_col* probe_key, int64_t n_build, int64_t n_probe, int64_t key_lo,
                                  int64_t key_hi, uint32_t routes, hs_join_table* out) {
    if (!build_key || !probe_key || !out || n_build < 0 || n_probe < 0) {
        hs_set_error("hs_join_table_plan: bad arguments");
        return HS_E_ARG;
    }
    const auto wants = [&](int route) { return (routes & HS_JOIN_ROUTE_BIT(route)) != 0; };
    const bool rows = n_build > 0 && n_probe > 0;
    const bool i32 = rows && build_key->kind == HS_I32 && probe_key->kind == HS_I32 &&
                     !(((uintptr_t)build_key->data | (uintptr_t)probe_key->data) & 15);
    hs_join_table t{};
    t.n_build = n_build;
    int64_t size[4] = {0, (int64_t)n_build * 4, (int64_t)n_build * 4, -1};  // bytes of every part (-1: no such part)
    const int64_t range = key_hi - key_lo + 1;
    if (wants(HS_JOIN_ROUTE_DENSE) && i32 && n_build < ((int64_t)1 << 31) && key_lo <= key_hi &&
        range <= std::min<int64_t>((int64_t)1 << 29, 32 * n_build + 65536) && range * 4 >= n_build && hs_join_dense_ws_bytes(n_build, range)) {
        t.route = HS_JOIN_ROUTE_DENSE;
        t.key_min = (int32_t)key_lo;
        t.slots = range;
        t.ws_bytes = (int64_t)hs_join_dense_ws_bytes(n_build, range);
        size[0] = range * 4;
    } else if (wants(HS_JOIN_ROUTE_HASH) && i32 && hs_join_hash_slots(n_build) > 0) {
        t.route = HS_JOIN_ROUTE_HASH;
        t.slots = hs_join_hash_slots(n_build);
        t.ws_bytes = (int64_t)hs_join_hash_ws_bytes(n_build);
        size[0] = t.slots * 8;
    } else if (wants(HS_JOIN_ROUTE_HASH_STR) && rows && build_key->kind == HS_STR && probe_key->kind == HS_STR &&
               hs_join_hash_str_slots(n_build) > 0) {
        t.route = HS_JOIN_ROUTE_HASH_STR;
        t.slots = hs_join_hash_str_slots(n_build);
        t.ws_bytes = (int64_t)hs_join_hash_str_ws_bytes(n_build);
        size[0] = t.slots * 8;
    } else if (wants(HS_JOIN_ROUTE_GLOBAL)) {
        t.route = HS_JOIN_ROUTE_GLOBAL;
        for (t.slots = 16; t.slots < 2 * n_build; t.slots *= 2) {}
        t.ws_bytes = (int64_t)hs_join_build_ws_bytes(n_build, t.slots);
        size[0] = size[1] = t.slots * 8;
        size[2] = (t.slots + 1) * 8;
        size[3] = (n_build > 0 ? n_build : 1) * 8;
    }
    for (int i = 0; i < 4 && t.route && size[i] >= 0; ++i) {
        t.part[i] = t.table_bytes;
        t.table_bytes = (t.table_bytes + size[i] + 64 + 255) & ~(int64_t)255;
    }
    *out = t;
    return HS_OK;
}

extern "C" int hs_join_table_build(void* stream, const hs_join_table* t, const hs_col* build_key, void* table, void* ws, uint32_t* status,
                                   uint32_t* flags) {
    if (!jt_args("hs_join_table_build", t, build_key, build_key, table)) return HS_E_ARG;
    const JtParts P(*t, table);
    uint32_t *const rows = P.at<uint32_t>(1), *const list_count = P.at<uint32_t>(2);
    switch (t->route) {
        case HS_JOIN_ROUTE_DENSE:
            return hs_join_dense_build(stream, (const int32_t*)build_key->data, t->n_build, t->key_min, t->slots, P.at<uint32_t>(0), rows,
                                       list_count, ws, flags);
        case HS_JOIN_ROUTE_HASH:
            return hs_join_hash_build(stream, (const int32_t*)build_key->data, t->n_build, P.p[0], rows, list_count, ws, status, flags);
        case HS_JOIN_ROUTE_HASH_STR:
            return hs_join_hash_str_build(stream, build_key, t->n_build, P.p[0], rows, list_count, ws, status, flags);
        default:
            return hs_join_build(stream, build_key, t->n_build, t->slots, P.at<uint64_t>(0), P.at<int64_t>(1), P.at<int64_t>(2),
                                 P.at<int64_t>(3), ws, flags);
    }
}

extern "C" int hs_join_table_count(void* stream, const hs_join_table* t, const hs_col* build_key, const hs_col* probe_key, int64_t n_probe,
                                   const void* table, int64_t* counts, void* aux) {
    if (!jt_args("hs_join_table_count", t, build_key, probe_key, table)) return HS_E_ARG;
    const JtParts P(*t, table);
    const uint32_t *const rows = P.at<uint32_t>(1), *const list_count = P.at<uint32_t>(2);
    switch (t->route) {
        case HS_JOIN_ROUTE_DENSE:
            return hs_join_dense_count(stream, (const int32_t*)probe_key->data, n_probe, t->key_min, t->slots, P.at<uint32_t>(0), rows,
                                       list_count, counts, aux);
        case HS_JOIN_ROUTE_HASH:
            return hs_join_hash_count(stream, (const int32_t*)probe_key->data, n_probe, t->n_build, P.p[0], rows, list_count, counts, aux);
        case HS_JOIN_ROUTE_HASH_STR:
            return hs_join_hash_str_count(stream, build_key, probe_key, n_probe, t->n_build, P.p[0], rows, list_count, counts, aux);
        default:
            return hs_join_count(stream, build_key, probe_key, n_probe, t->slots, P.at<uint64_t>(0), P.at<int64_t>(1), P.at<int64_t>(2),
                                 counts);
    }
}

extern "C" int hs_join_table_fill(void* stream, const hs_join_table* t, const hs_col* build_key, const hs_col* probe_key, int64_t n_probe,
                                  const void* table, const void* aux, const int64_t* out_start, int64_t* out_left, int64_t* out_right) {
    if (!jt_args("hs_join_table_fill", t, build_key, probe_key, table)) return HS_E_ARG;
    const JtParts P(*t, table);
    if (t->route != HS_JOIN_ROUTE_GLOBAL) return hs_join_dense_fill(stream, n_probe, P.at<uint32_t>(1), aux, out_start, out_left, out_right);
    return hs_join_fill(stream, build_key, probe_key, n_probe, t->slots, P.at<uint64_t>(0), P.at<int64_t>(1), P.at<int64_t>(2),
                        P.at<int64_t>(3), out_start, out_left, out_right);
}
