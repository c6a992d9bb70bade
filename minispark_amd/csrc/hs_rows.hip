// hs_rows.hip - the row-forming pass in front of the radix (HBM) aggregation tier.
//
// The radix tier (hs_radix.hip) takes its input by POSITION: a key column, unit bounds as positions and one value column
// per aggregate.  A stage has table columns and ONE program `[filter ... FILTER]* KEY [argument ... AGG acc]*`.  This pass
// goes from the one to the other: the rows that pass every filter, in ascending row order, as a dense key column, the
// bare stored argument columns in their stored width and every computed argument as the 64-bit cell the interpreter
// yields.  It replaces the per-operator sequence hs_eval (mask) -> hs_compact -> one hs_gather_fixed per stored column ->
// hs_eval (computed arguments) of the Python engine (device.py aggregate_partial_global) - reference FilterTask.execute
// tasks.py:167-177 and the argument evaluation of fill_aggregators tasks.py:295-310.
//
// Two sweeps when there is a WHERE (one without): the count sweep runs the filter part of the program over the filters'
// columns only and leaves one count per SEGMENT (the rows a 4096-row tile shares with one unit), an exclusive scan turns
// the counts into segment starts, the write sweep runs the whole program and stores every survivor at
// start + rank.  Ranks come from ballots inside a wave and from the waves' counts through LDS: no atomic decides a
// position, so the output is the same on every run.  Loads are the scan kernel's (hs_agg_kernel.h): four consecutive rows
// per lane, 16-byte loads, the next step's loads issued before this step is evaluated.  The operators are the
// interpreter's (hs_bin<> in hs_device.h): a new Sink, nothing else.
#include <stdint.h>
#include <string.h>

#include "hs_agg_kernel.h"

void hs_set_error(const char* fmt, ...);

#define ROWS_CHECK_LAUNCH(name)                                                            \
    do {                                                                                   \
        const hipError_t e_ = hipGetLastError();                                           \
        if (e_ != hipSuccess) {                                                            \
            hs_set_error("%s: kernel launch failed (%s)", name, hipGetErrorString(e_));    \
            return HS_E_LAUNCH;                                                            \
        }                                                                                  \
    } while (0)

namespace {

constexpr int ROWS_WG = 256;
constexpr int ROWS_STEP = ROWS_WG * HS_V;      // rows of one step of a workgroup
constexpr int ROWS_STEPS = 4;
constexpr int ROWS_TILE = ROWS_STEP * ROWS_STEPS;  // 4096 rows, aligned: a segment never leaves its tile

struct RowsArgs {
    HsCols cols;
    hs_program prog;
    int32_t key_slot, n_units;
    uint32_t key_pc;     // index of HS_OP_KEY: the count sweep stops in front of it
    uint32_t load_mask;  // bit c: slot c is preloaded by this sweep
    int32_t compact;     // write sweep: 1 = position from the segment starts, 0 = position is the row (no filter)
    int32_t vec;         // every preloaded column is 16-byte aligned
    int64_t n_rows, n_segs_max;
    const int64_t* unit_rows;  // [n_units + 1]
    const int64_t* seg0;       // [n_units + 1] segments before unit u
    int64_t* seg_count;        // count sweep: [n_segs_max]
    const int64_t* seg_start;  // write sweep: [n_segs_max + 1]
    void* out_key;
    void* out_vals[HS_MAX_ACC];
    int32_t val_kinds[HS_MAX_ACC];
    int64_t* out_bounds;
    uint32_t* flags;
};

struct RowsCells {
    uint64_t cell[HS_FUSED_COLS][HS_V];
};

// one row of a preloadable column as the cell hs_load_quad gives it (the last, partial quad of a table and unaligned buffers)
__device__ __forceinline__ uint64_t rows_load_one(const hs_col& c, int64_t row) {
    if (c.kind != HS_STR) return hs_load_cell(c, row);
    const uint8_t* p = (const uint8_t*)c.data + row * (int64_t)c.fixed_len;
    uint64_t k = (uint64_t)c.fixed_len << 56;
    for (int i = 0; i < c.fixed_len; ++i) k |= (uint64_t)p[i] << (8 * i);
    return k;
}

__device__ __forceinline__ void rows_load(const RowsArgs& A, int64_t row0, int64_t hi, RowsCells& x) {
#pragma unroll
    for (int c = 0; c < HS_FUSED_COLS; ++c) {
        if (!((A.load_mask >> c) & 1u)) continue;  // wave-uniform
        const hs_col& col = A.cols.c[c];
        if (row0 >= hi) {
#pragma unroll
            for (int j = 0; j < HS_V; ++j) x.cell[c][j] = 0;
        } else if (A.vec && row0 + HS_V <= A.n_rows) {
            hs_load_quad(col, row0, x.cell[c]);
        } else {
#pragma unroll
            for (int j = 0; j < HS_V; ++j) x.cell[c][j] = row0 + j < A.n_rows ? rows_load_one(col, row0 + j) : 0;
        }
    }
}

// the segment of this workgroup: unit, rows [lo, hi) and the aligned tile they lie in
struct RowsSeg {
    int32_t unit;
    int64_t tile0, lo, hi;
};
__device__ __forceinline__ bool rows_segment(const RowsArgs& A, int64_t s, RowsSeg& g) {
    if (s >= A.seg0[A.n_units]) return false;
    int32_t a = 0, b = A.n_units;  // seg0[a] <= s < seg0[b]
    while (b - a > 1) {
        const int32_t m = a + (b - a) / 2;
        if (A.seg0[m] <= s) a = m;
        else b = m;
    }
    g.unit = a;
    int64_t ub = A.unit_rows[a], ue = A.unit_rows[a + 1];
    ub = ub < 0 ? 0 : ub;
    ue = ue > A.n_rows ? A.n_rows : ue;
    g.tile0 = (ub / ROWS_TILE + (s - A.seg0[a])) * ROWS_TILE;
    g.lo = ub > g.tile0 ? ub : g.tile0;
    g.hi = ue < g.tile0 + ROWS_TILE ? ue : g.tile0 + ROWS_TILE;
    if (g.hi < g.lo) g.hi = g.lo;  // an empty unit: a segment of no rows (it still owns its out_bounds entry)
    return true;
}

template <bool COUNT>
struct RowsSink {
    const RowsArgs& A;
    const RowsCells& x;
    int64_t row0;
    bool alive[HS_V];
    int64_t pos[HS_V];
    int64_t base;       // write sweep: output position of the step's first survivor
    uint32_t step_total;
    int32_t* wave_cnt;  // LDS [ROWS_WG / HS_WAVE]
    __device__ __forceinline__ RowsSink(const RowsArgs& a, const RowsCells& c, int32_t* w) : A(a), x(c), wave_cnt(w) {}
    __device__ __forceinline__ void load(uint32_t s, uint64_t (&dst)[HS_V]) const {
        switch (s) {
#define HS_CASE(K)                                                          \
    case K:                                                                 \
        _Pragma("unroll") for (int j = 0; j < HS_V; ++j) dst[j] = x.cell[K][j]; \
        break;
            HS_CASE(0) HS_CASE(1) HS_CASE(2) HS_CASE(3) HS_CASE(4) HS_CASE(5) HS_CASE(6) HS_CASE(7)
#undef HS_CASE
            default: break;
        }
    }
    __device__ __forceinline__ uint64_t load(uint32_t s, int j) const {
        uint64_t tmp[HS_V];
        load(s, tmp);
        return tmp[j];
    }
    __device__ __forceinline__ bool live(int j) const { return alive[j]; }
    __device__ __forceinline__ int64_t row(int j) const { return row0 + j; }
    __device__ __forceinline__ void filter(int j, bool keep) { alive[j] = alive[j] && keep; }
    __device__ __forceinline__ void out(uint32_t, int, uint64_t) {}
    // survivors of the wave in front of this lane's rows, and of the whole wave: rows ascend with the lane, then with j
    __device__ __forceinline__ void wave_ranks(uint32_t& before, uint32_t& total) const {
        const uint64_t lt = (1ull << (threadIdx.x & (HS_WAVE - 1))) - 1ull;
        before = total = 0;
#pragma unroll
        for (int j = 0; j < HS_V; ++j) {
            const uint64_t m = __ballot(alive[j]);
            before += (uint32_t)__popcll(m & lt);
            total += (uint32_t)__popcll(m);
        }
    }
    __device__ __forceinline__ void key() {
        if constexpr (COUNT) return;
        if (A.compact) {
            uint32_t before, total;
            wave_ranks(before, total);
            const int w = threadIdx.x / HS_WAVE;
            if ((threadIdx.x & (HS_WAVE - 1)) == 0) wave_cnt[w] = (int32_t)total;
            __syncthreads();
            uint32_t wave_base = 0, all = 0;
#pragma unroll
            for (int k = 0; k < ROWS_WG / HS_WAVE; ++k) {
                const uint32_t c = (uint32_t)wave_cnt[k];
                if (k < w) wave_base += c;
                all += c;
            }
            __syncthreads();  // (the next step writes wave_cnt again)
            step_total = all;
            int64_t p = base + wave_base + before;
#pragma unroll
            for (int j = 0; j < HS_V; ++j) {
                pos[j] = p;
                p += alive[j] ? 1 : 0;
            }
        } else {
#pragma unroll
            for (int j = 0; j < HS_V; ++j) pos[j] = row0 + j;
        }
#pragma unroll
        for (int j = 0; j < HS_V; ++j) alive[j] = alive[j] && pos[j] < A.n_rows;  // (never: malformed unit bounds only)
        if (!A.out_key) return;
        const hs_col& kc = A.cols.c[A.key_slot];
        if (kc.kind == HS_STR && !hs_str_preloads(kc)) {  // other fixed lengths: the bytes where they lie
            const int64_t len = kc.fixed_len;
#pragma unroll
            for (int j = 0; j < HS_V; ++j) {
                if (!alive[j]) continue;
                const uint8_t* src = (const uint8_t*)kc.data + (row0 + j) * len;
                uint8_t* dst = (uint8_t*)A.out_key + pos[j] * len;
                for (int64_t i = 0; i < len; ++i) dst[i] = src[i];
            }
            return;
        }
        uint64_t kcell[HS_V];
        load((uint32_t)A.key_slot, kcell);
#pragma unroll
        for (int j = 0; j < HS_V; ++j) {
            if (!alive[j]) continue;
            const uint64_t v = kcell[j];
            switch (kc.kind) {
                case HS_I32: ((int32_t*)A.out_key)[pos[j]] = (int32_t)(int64_t)v; break;
                case HS_F32: ((float*)A.out_key)[pos[j]] = (float)hs_u2d(v); break;  // (widening a float is exact both ways)
                case HS_STR:
                    if (kc.fixed_len == 1) ((uint8_t*)A.out_key)[pos[j]] = (uint8_t)v;
                    else if (kc.fixed_len == 2) ((uint16_t*)A.out_key)[pos[j]] = (uint16_t)v;
                    else ((uint32_t*)A.out_key)[pos[j]] = (uint32_t)v;
                    break;
                default: ((uint64_t*)A.out_key)[pos[j]] = v; break;
            }
        }
    }
    __device__ __forceinline__ void agg(uint32_t a, int j, uint64_t v) {
        if constexpr (COUNT) return;
        void* o = A.out_vals[a];
        if (!o || !alive[j]) return;
        switch (A.val_kinds[a]) {
            case HS_I32: ((int32_t*)o)[pos[j]] = (int32_t)(int64_t)v; break;
            case HS_F32: ((float*)o)[pos[j]] = (float)hs_u2d(v); break;
            default: ((uint64_t*)o)[pos[j]] = v; break;
        }
    }
};

// instructions [first, last) of the program over one row quad (InterpProg::run's loop: LD moves the quad with one switch)
template <int D, class Sink>
__device__ __forceinline__ void rows_run(const RowsArgs& A, uint32_t first, uint32_t last, Sink& sink, uint32_t& err) {
    const hs_program& P = A.prog;
    uint64_t st[D][HS_V];
#pragma unroll
    for (int d = 0; d < D; ++d)
#pragma unroll
        for (int j = 0; j < HS_V; ++j) st[d][j] = 0;
    for (uint32_t pc = first; pc < last; ++pc) {
        const uint64_t w = P.ins[pc];
        const uint32_t sp = hs_ins_sp(w);
        if (hs_ins_op(w) == HS_OP_LD) {
            uint64_t tmp[HS_V];
            sink.load(hs_ins_a(w), tmp);
            switch (sp) {
#define HS_PUSH(K)                                                            \
    case K:                                                                   \
        if constexpr (K < D) {                                                \
            _Pragma("unroll") for (int j = 0; j < HS_V; ++j) st[K][j] = tmp[j]; \
        }                                                                     \
        break;
                HS_PUSH(0) HS_PUSH(1) HS_PUSH(2) HS_PUSH(3) HS_PUSH(4) HS_PUSH(5) HS_PUSH(6) HS_PUSH(7)
#undef HS_PUSH
                default: err |= HS_FLAG_BAD_PROGRAM; break;
            }
            continue;
        }
        switch (sp) {
            case 0: hs_exec_at<0, D, HS_V>(w, P, A.cols, st, sink, err); break;
            case 1: hs_exec_at<1, D, HS_V>(w, P, A.cols, st, sink, err); break;
            case 2: hs_exec_at<2, D, HS_V>(w, P, A.cols, st, sink, err); break;
            case 3: hs_exec_at<3, D, HS_V>(w, P, A.cols, st, sink, err); break;
            case 4: hs_exec_at<4, D, HS_V>(w, P, A.cols, st, sink, err); break;
            default:
                if constexpr (D > 4) {
                    switch (sp) {
                        case 5: hs_exec_at<5, D, HS_V>(w, P, A.cols, st, sink, err); break;
                        case 6: hs_exec_at<6, D, HS_V>(w, P, A.cols, st, sink, err); break;
                        case 7: hs_exec_at<7, D, HS_V>(w, P, A.cols, st, sink, err); break;
                        case 8: hs_exec_at<8, D, HS_V>(w, P, A.cols, st, sink, err); break;
                        default: err |= HS_FLAG_BAD_PROGRAM; break;
                    }
                } else {
                    err |= HS_FLAG_BAD_PROGRAM;
                }
                break;
        }
    }
}

// One workgroup per segment.  COUNT: survivors of the segment -> seg_count[s] (0 for the unused tail of the grid's range).
// Else: the whole program; survivors leave at seg_start[s] + rank (or at their row), out_bounds from the segment starts.
template <int D, bool COUNT>
__global__ void __launch_bounds__(ROWS_WG) k_agg_rows(const RowsArgs A_kernarg) {
    HS_KERNARG(RowsArgs, A);
    __shared__ int32_t wave_cnt[ROWS_WG / HS_WAVE];
    const int64_t s = blockIdx.x;
    RowsSeg g;
    if (!rows_segment(A, s, g)) {
        if (COUNT && threadIdx.x == 0) A.seg_count[s] = 0;
        return;
    }
    RowsCells cur, nxt;
    RowsSink<COUNT> sink(A, cur, wave_cnt);
    sink.base = (!COUNT && A.compact) ? A.seg_start[s] : 0;
    sink.step_total = 0;
    if (!COUNT && A.compact && A.out_bounds && threadIdx.x == 0) {
        if (s == A.seg0[g.unit]) A.out_bounds[g.unit] = sink.base;
        if (s + 1 == A.seg0[A.n_units]) A.out_bounds[A.n_units] = A.seg_start[A.n_segs_max];
    }
    uint32_t err = 0, counted = 0;
    // the steps of the tile that hold rows of the segment (wave-uniform: every lane of the workgroup runs the same steps)
    const int step_lo = g.hi > g.lo ? (int)((g.lo - g.tile0) / ROWS_STEP) : 0;
    const int step_hi = g.hi > g.lo ? (int)((g.hi - 1 - g.tile0) / ROWS_STEP) + 1 : 0;
    const int64_t lane0 = g.tile0 + (int64_t)threadIdx.x * HS_V;
    if (step_lo < step_hi) rows_load(A, lane0 + (int64_t)step_lo * ROWS_STEP, g.hi, cur);
    for (int step = step_lo; step < step_hi; ++step) {
        const int64_t row0 = lane0 + (int64_t)step * ROWS_STEP;
        if (step + 1 < step_hi) rows_load(A, row0 + ROWS_STEP, g.hi, nxt);  // in flight while this step is evaluated
        sink.row0 = row0;
#pragma unroll
        for (int j = 0; j < HS_V; ++j) sink.alive[j] = row0 + j >= g.lo && row0 + j < g.hi;
        if constexpr (COUNT) {
            rows_run<D>(A, 0, A.key_pc, sink, err);
            uint32_t before, total;
            sink.wave_ranks(before, total);
            counted += total;
        } else {
            rows_run<D>(A, 0, A.prog.n_ins, sink, err);
            sink.base += sink.step_total;
        }
        if (step + 1 < step_hi) cur = nxt;
    }
    if constexpr (COUNT) {
        if ((threadIdx.x & (HS_WAVE - 1)) == 0) wave_cnt[threadIdx.x / HS_WAVE] = (int32_t)counted;
        __syncthreads();
        if (threadIdx.x == 0) {
            int64_t all = 0;
            for (int k = 0; k < ROWS_WG / HS_WAVE; ++k) all += wave_cnt[k];
            A.seg_count[s] = all;
        }
    } else {
        if (err) atomicOr(A.flags, err);  // raised by surviving rows only (sink.live gates hs_bin's error reports)
    }
}

// segments of every unit: the 4096-row tiles it touches, one (of no rows) for an empty unit
__global__ void __launch_bounds__(256) k_rows_unit_segs(const int64_t* unit_rows, int32_t n_units, int64_t n_rows, int64_t* segs) {
    for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < n_units; u += (int64_t)gridDim.x * blockDim.x) {
        int64_t b = unit_rows[u], e = unit_rows[u + 1];
        b = b < 0 ? 0 : b;
        e = e > n_rows ? n_rows : e;
        segs[u] = e > b ? (e - 1) / ROWS_TILE - b / ROWS_TILE + 1 : 1;
    }
}

int64_t rows_max_segs(int64_t n_rows, int32_t n_units) { return n_rows / ROWS_TILE + 2 * (int64_t)n_units + 2; }
size_t rows_align(size_t b) { return (b + 255) & ~(size_t)255; }

// the shape of a stage program: filters, KEY, then one argument + AGG per accumulator
struct RowsShape {
    uint32_t key_pc = 0;
    int n_filters = 0, depth = 0;
    uint32_t filter_slots = 0, all_slots = 0;
    uint32_t arg_first[HS_MAX_ACC] = {}, arg_last[HS_MAX_ACC] = {};  // instructions [first, last) in front of AGG a
};

int rows_shape(const char* who, const hs_col* cols, int32_t n_cols, int32_t key_slot, const hs_program* prog, const hs_agg_spec* spec,
               RowsShape& S) {
    if (!prog || !spec || (n_cols > 0 && !cols) || n_cols < 1 || n_cols > HS_MAX_COLS || key_slot < 0 || key_slot >= n_cols ||
        spec->n_acc < 0 || spec->n_acc > HS_MAX_ACC) {
        hs_set_error("%s: bad arguments", who);
        return HS_E_ARG;
    }
    if (prog->n_ins > HS_MAX_INS || prog->n_lit > HS_MAX_LIT) {
        hs_set_error("%s: program too long", who);
        return HS_E_LIMIT;
    }
    if (hs_refuse_narrow(who, cols, n_cols)) return HS_E_ARG;
    bool have_key = false;
    bool seen[HS_MAX_ACC] = {};
    uint32_t arg0 = 0;
    for (uint32_t pc = 0; pc < prog->n_ins; ++pc) {
        const uint64_t w = prog->ins[pc];
        const uint32_t op = (uint32_t)(w & 0xff), sp = (uint32_t)((w >> 8) & 0xff), a = (uint32_t)((w >> 16) & 0xffff);
        if ((int)sp + 1 > S.depth) S.depth = (int)sp + 1;
        if (op == HS_OP_END) break;
        if (op == HS_OP_LD) {
            if ((int)a >= n_cols || cols[a].kind == HS_STR || a >= HS_FUSED_COLS) {
                hs_set_error("%s: LD of slot %u (numeric slots 0 .. %d of %d columns)", who, a, HS_FUSED_COLS - 1, n_cols);
                return HS_E_ARG;
            }
            if (cols[a].kind & HS_PAIR) {
                hs_set_error("%s: pair-indexed columns are not read here (hand over gathered columns)", who);
                return HS_E_LIMIT;
            }
            S.all_slots |= 1u << a;
            if (!have_key) S.filter_slots |= 1u << a;
        } else if (op == HS_OP_FILTER) {
            if (have_key) {
                hs_set_error("%s: FILTER behind KEY", who);
                return HS_E_ARG;
            }
            ++S.n_filters;
        } else if (op == HS_OP_KEY) {
            if (have_key) {
                hs_set_error("%s: two KEY instructions", who);
                return HS_E_ARG;
            }
            have_key = true;
            S.key_pc = pc;
            arg0 = pc + 1;
        } else if (op == HS_OP_AGG) {
            if (!have_key || (int)a >= spec->n_acc || seen[a]) {
                hs_set_error("%s: AGG %u in front of KEY, twice, or beyond the %d accumulators", who, a, spec->n_acc);
                return HS_E_ARG;
            }
            seen[a] = true;
            S.arg_first[a] = arg0;
            S.arg_last[a] = pc;
            arg0 = pc + 1;
        } else if (op == HS_OP_OUT) {
            hs_set_error("%s: OUT in an aggregate program", who);
            return HS_E_ARG;
        }
    }
    for (int a = 0; a < spec->n_acc; ++a)
        if (!seen[a]) have_key = false;
    if (!have_key) {
        hs_set_error("%s: the program is not [filter ... FILTER]* KEY [argument ... AGG a]* over %d accumulators", who, spec->n_acc);
        return HS_E_ARG;
    }
    const hs_col& kc = cols[key_slot];
    const bool key_ok = kc.kind == HS_I32 || kc.kind == HS_F32 || kc.kind == HS_I64 || (kc.kind == HS_STR && kc.fixed_len >= 1);
    if (!key_ok) {
        hs_set_error("%s: the key column must be INTEGER / FLOAT / TIMESTAMP as stored or a STRING of one fixed length", who);
        return HS_E_LIMIT;
    }
    return HS_OK;
}

}  // namespace

// How every aggregate argument travels to the radix tier, from the program alone: -1 a literal (const_cells[a] = its
// cell, nothing is written), HS_I32 / HS_F32 / HS_I64 a bare stored column (val_slots[a] = its slot), HS_F64 / HS_I64 the
// expression's cell (val_slots[a] = -1).  Host only.
extern "C" int hs_agg_rows_classify(const hs_col* cols, int32_t n_cols, int32_t key_slot, const hs_program* prog,
                                    const hs_agg_spec* spec, int32_t* val_kinds, int32_t* val_slots, uint64_t* const_cells,
                                    int32_t* n_filters) {
    RowsShape S;
    const int rc = rows_shape("hs_agg_rows_classify", cols, n_cols, key_slot, prog, spec, S);
    if (rc) return rc;
    if (spec->n_acc > 0 && (!val_kinds || !val_slots || !const_cells)) {
        hs_set_error("hs_agg_rows_classify: bad arguments");
        return HS_E_ARG;
    }
    for (int a = 0; a < spec->n_acc; ++a) {
        const bool is_int = spec->is_int[a] != 0;
        val_kinds[a] = is_int ? HS_I64 : HS_F64;
        val_slots[a] = -1;
        const_cells[a] = 0;
        if (S.arg_last[a] - S.arg_first[a] != 1) continue;
        const uint64_t w = prog->ins[S.arg_first[a]];
        const uint32_t op = (uint32_t)(w & 0xff), x = (uint32_t)((w >> 16) & 0xffff);
        if (op == HS_OP_LIT && x < prog->n_lit) {
            val_kinds[a] = -1;
            const_cells[a] = prog->lit[x];
        } else if (op == HS_OP_LD) {
            const int kind = cols[x].kind;
            if ((kind == HS_F32 && !is_int) || ((kind == HS_I32 || kind == HS_I64) && is_int)) {
                val_kinds[a] = kind;
                val_slots[a] = (int32_t)x;
            }
        }
    }
    if (n_filters) *n_filters = S.n_filters;
    return HS_OK;
}

extern "C" size_t hs_agg_rows_ws_bytes(int64_t n_rows, int32_t n_units) {
    if (n_rows < 0) n_rows = 0;
    if (n_units < 0) n_units = 0;
    const int64_t segs = rows_max_segs(n_rows, n_units);
    const int64_t scan_n = segs > n_units ? segs : n_units;
    return 2 * rows_align((size_t)(n_units + 1) * 8) + 2 * rows_align((size_t)(segs + 1) * 8) + rows_align(hs_scan_ws_bytes(scan_n));
}

extern "C" int hs_agg_rows(void* stream_, const hs_col* cols, int32_t n_cols, int32_t key_slot, const hs_program* prog,
                           const hs_agg_spec* spec, const int64_t* unit_rows, int32_t n_units, int64_t n_rows, void* out_key,
                           void* const* out_vals, const int32_t* out_val_kinds, int64_t* out_bounds, void* ws_, uint32_t* flags) {
    RowsShape S;
    const int rc0 = rows_shape("hs_agg_rows", cols, n_cols, key_slot, prog, spec, S);
    if (rc0) return rc0;
    if (!unit_rows || n_units < 0 || n_rows < 0 || !out_bounds || !ws_ || !flags || ((uintptr_t)ws_ & 15) ||
        (spec->n_acc > 0 && (!out_vals || !out_val_kinds))) {
        hs_set_error("hs_agg_rows: bad arguments");
        return HS_E_ARG;
    }
    hipStream_t stream = (hipStream_t)stream_;
    if (n_units == 0) {
        hs_memset_async(out_bounds, 0, 8, stream);
        return HS_OK;
    }
    RowsArgs A;
    memset(&A, 0, sizeof(A));
    A.cols.n = n_cols;
    for (int i = 0; i < HS_MAX_COLS; ++i) A.cols.c[i] = i < n_cols ? cols[i] : hs_col{HS_U8, -1, nullptr, nullptr, nullptr};
    A.prog = *prog;
    A.key_slot = key_slot;
    A.n_units = n_units;
    A.key_pc = S.key_pc;
    A.n_rows = n_rows;
    A.out_key = out_key;
    A.out_bounds = out_bounds;
    A.flags = flags;
    // the caller's kinds must be what the program says, or the (always correct) cell
    int32_t kinds[HS_MAX_ACC], slots[HS_MAX_ACC];
    uint64_t cells[HS_MAX_ACC];
    const int rc1 = hs_agg_rows_classify(cols, n_cols, key_slot, prog, spec, kinds, slots, cells, nullptr);
    if (rc1) return rc1;
    for (int a = 0; a < spec->n_acc; ++a) {
        const int32_t cell_kind = spec->is_int[a] ? HS_I64 : HS_F64;
        if (out_val_kinds[a] != kinds[a] && out_val_kinds[a] != cell_kind) {
            hs_set_error("hs_agg_rows: accumulator %d cannot travel as kind %d (the program says %d)", a, (int)out_val_kinds[a], (int)kinds[a]);
            return HS_E_ARG;
        }
        A.val_kinds[a] = out_val_kinds[a];
        A.out_vals[a] = out_val_kinds[a] < 0 ? nullptr : out_vals[a];
    }
    const hs_col& kc = cols[key_slot];
    const bool key_pre = kc.kind != HS_STR || kc.fixed_len == 1 || kc.fixed_len == 2 || kc.fixed_len == 4;  // (hs_str_preloads)
    if (key_pre && key_slot >= HS_FUSED_COLS) {
        hs_set_error("hs_agg_rows: the key column must lie in slots 0 .. %d", HS_FUSED_COLS - 1);
        return HS_E_ARG;
    }
    const uint32_t key_bit = (out_key && key_pre) ? 1u << key_slot : 0u;
    auto aligned = [&](uint32_t mask) {
        for (int c = 0; c < HS_FUSED_COLS; ++c)
            if (((mask >> c) & 1u) && ((uintptr_t)cols[c].data & 15)) return 0;
        return 1;
    };
    uint8_t* ws = (uint8_t*)ws_;
    const int64_t segs = rows_max_segs(n_rows, n_units);
    int64_t* unit_segs = (int64_t*)ws;
    int64_t* seg0 = (int64_t*)(ws + rows_align((size_t)(n_units + 1) * 8));
    int64_t* seg_count = (int64_t*)((uint8_t*)seg0 + rows_align((size_t)(n_units + 1) * 8));
    int64_t* seg_start = (int64_t*)((uint8_t*)seg_count + rows_align((size_t)(segs + 1) * 8));
    void* scan_ws = (uint8_t*)seg_start + rows_align((size_t)(segs + 1) * 8);
    A.n_segs_max = segs;
    A.unit_rows = unit_rows;
    A.seg0 = seg0;
    A.seg_count = seg_count;
    A.seg_start = seg_start;
    const unsigned ugrid = (unsigned)((n_units + 255) / 256 > 1024 ? 1024 : (n_units + 255) / 256);
    hipLaunchKernelGGL(k_rows_unit_segs, dim3(ugrid), dim3(256), 0, stream, unit_rows, n_units, n_rows, unit_segs);
    ROWS_CHECK_LAUNCH("hs_agg_rows (segments)");
    int rc = hs_exclusive_scan_i64(stream, unit_segs, n_units, seg0, scan_ws);
    if (rc) return rc;
    const bool deep = S.depth > 4;
    if (S.n_filters > 0) {
        A.compact = 1;
        A.load_mask = S.filter_slots;
        A.vec = aligned(A.load_mask);
        if (deep) hipLaunchKernelGGL((k_agg_rows<HS_MAX_STACK, true>), dim3((unsigned)segs), dim3(ROWS_WG), 0, stream, A);
        else hipLaunchKernelGGL((k_agg_rows<4, true>), dim3((unsigned)segs), dim3(ROWS_WG), 0, stream, A);
        ROWS_CHECK_LAUNCH("hs_agg_rows (count sweep)");
        rc = hs_exclusive_scan_i64(stream, seg_count, segs, seg_start, scan_ws);
        if (rc) return rc;
    } else {
        A.compact = 0;  // position = row: the bounds are the unit boundaries themselves
        if (hipMemcpyAsync(out_bounds, unit_rows, (size_t)(n_units + 1) * 8, hipMemcpyDeviceToDevice, stream) != hipSuccess) {
            hs_set_error("hs_agg_rows: copy of the unit boundaries failed");
            return HS_E_LAUNCH;
        }
    }
    A.load_mask = S.all_slots | key_bit;
    A.vec = aligned(A.load_mask);
    if (deep) hipLaunchKernelGGL((k_agg_rows<HS_MAX_STACK, false>), dim3((unsigned)segs), dim3(ROWS_WG), 0, stream, A);
    else hipLaunchKernelGGL((k_agg_rows<4, false>), dim3((unsigned)segs), dim3(ROWS_WG), 0, stream, A);
    ROWS_CHECK_LAUNCH("hs_agg_rows (write sweep)");
    return HS_OK;
}

// =====================================================================================================
// Composite GROUP BY keys: hs_key_pack / hs_key_unpack
// =====================================================================================================
// Row r of the packed column is the bytes of the key parts of row r, back to back: a column-to-row transposition of byte
// runs.  A workgroup takes a tile of HS_KEY_TILE_ROWS rows through LDS (at most 16 KiB): every part is read as the
// contiguous byte range of the tile with 16-byte loads and laid into the tile image at row * width + offset, then the
// image - contiguous in the output as well - leaves with 16-byte stores.  The unpack runs the same two steps the other
// way round.  A tuple made of single bytes only (dictionary codes) skips LDS: k_key_pack_bytes.  Buffers of the engine carry 64 bytes of slack and start 16-byte aligned, so the last vector of a part's
// range may be read past its last row; a source that is not aligned is read byte by byte.  Nothing is written past the
// last row.
namespace {

struct KeyArgs {
    const uint8_t* part[HS_KEY_MAX_PARTS];  // pack: sources; unpack: destinations (written through key_dst)
    int32_t width[HS_KEY_MAX_PARTS];
    int32_t off[HS_KEY_MAX_PARTS];
    int32_t n_parts, W;
};

constexpr int KEY_WG = 256;

// bytes [16 v, 16 v + 16) of a part's tile range -> the tile image.  `e`: elements (rows) of the part in the tile.
__device__ __forceinline__ void key_scatter16(uint8_t* tile, const uint32_t w[4], int64_t v, int32_t pw, int32_t off, int32_t W,
                                              int32_t nbytes) {
    const int32_t b0 = (int32_t)v * 16;
    if (pw == 4 && !((W | off) & 3)) {  // whole words, word-aligned in the image
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (b0 + 4 * j < nbytes) *reinterpret_cast<uint32_t*>(tile + ((b0 >> 2) + j) * W + off) = w[j];
        return;
    }
    if (pw == 8 && !((W | off) & 3)) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (b0 + 4 * j < nbytes) *reinterpret_cast<uint32_t*>(tile + ((b0 >> 3) + (j >> 1)) * W + off + 4 * (j & 1)) = w[j];
        return;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int32_t b = b0 + j;
        if (b < nbytes) {
            const int32_t row = pw == 1 ? b : pw == 4 ? b >> 2 : pw == 8 ? b >> 3 : b / pw;
            tile[row * W + off + (b - row * pw)] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
        }
    }
}

__global__ void __launch_bounds__(KEY_WG) k_key_pack(const KeyArgs A, int64_t n, uint8_t* out) {
    __shared__ uint4 s_tile[HS_KEY_TILE_ROWS * HS_KEY_MAX_WIDTH / 16];
    uint8_t* tile = reinterpret_cast<uint8_t*>(s_tile);
    const int64_t n_tiles = (n + HS_KEY_TILE_ROWS - 1) / HS_KEY_TILE_ROWS;
    const int32_t W = A.W;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t row0 = t * HS_KEY_TILE_ROWS;
        const int32_t rows = (int32_t)(n - row0 < HS_KEY_TILE_ROWS ? n - row0 : HS_KEY_TILE_ROWS);
        for (int k = 0; k < A.n_parts; ++k) {
            const int32_t pw = A.width[k], off = A.off[k], nbytes = rows * pw;
            const uint8_t* src = A.part[k] + row0 * pw;  // row0 * pw is a multiple of 16: aligned iff the part is
            if (!((uintptr_t)src & 15)) {
                const int32_t nvec = (nbytes + 15) >> 4;
                for (int32_t v = threadIdx.x; v < nvec; v += KEY_WG) {
                    const uint4 x = *reinterpret_cast<const uint4*>(src + (int64_t)v * 16);  // (slack behind the last row)
                    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
                    key_scatter16(tile, w, v, pw, off, W, nbytes);
                }
            } else {
                for (int32_t b = threadIdx.x; b < nbytes; b += KEY_WG) {
                    const int32_t row = b / pw;
                    tile[row * W + off + (b - row * pw)] = src[b];
                }
            }
        }
        __syncthreads();
        const int32_t total = rows * W;
        uint8_t* dst = out + row0 * W;  // 16-byte aligned: `out` is, and row0 * W is a multiple of 16
        const int32_t full = total >> 4;
        for (int32_t v = threadIdx.x; v < full; v += KEY_WG) *reinterpret_cast<uint4*>(dst + (int64_t)v * 16) = s_tile[v];
        for (int32_t b = (full << 4) + threadIdx.x; b < total; b += KEY_WG) dst[b] = tile[b];  // the last rows' tail bytes
        __syncthreads();
    }
}

__global__ void __launch_bounds__(KEY_WG) k_key_unpack(const KeyArgs A, int64_t n, const int64_t* n_dev, const uint8_t* keys) {
    __shared__ uint4 s_tile[HS_KEY_TILE_ROWS * HS_KEY_MAX_WIDTH / 16];
    uint8_t* tile = reinterpret_cast<uint8_t*>(s_tile);
    if (n_dev) {
        const int64_t d = *n_dev;
        n = d < n ? (d < 0 ? 0 : d) : n;
    }
    const int64_t n_tiles = (n + HS_KEY_TILE_ROWS - 1) / HS_KEY_TILE_ROWS;
    const int32_t W = A.W;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t row0 = t * HS_KEY_TILE_ROWS;
        const int32_t rows = (int32_t)(n - row0 < HS_KEY_TILE_ROWS ? n - row0 : HS_KEY_TILE_ROWS);
        const int32_t total = rows * W;
        const uint8_t* src = keys + row0 * W;
        if (!((uintptr_t)src & 15)) {
            const int32_t nvec = (total + 15) >> 4;
            for (int32_t v = threadIdx.x; v < nvec; v += KEY_WG)
                s_tile[v] = *reinterpret_cast<const uint4*>(src + (int64_t)v * 16);  // (slack behind the last row)
        } else {
            for (int32_t b = threadIdx.x; b < total; b += KEY_WG) tile[b] = src[b];
        }
        __syncthreads();
        for (int k = 0; k < A.n_parts; ++k) {
            const int32_t pw = A.width[k], off = A.off[k], nbytes = rows * pw;
            uint8_t* dst = const_cast<uint8_t*>(A.part[k]) + row0 * pw;  // 16-byte aligned (hs_key_unpack checks the base)
            const int32_t full = nbytes >> 4;
            for (int32_t v = threadIdx.x; v < full; v += KEY_WG) {
                uint32_t o[4] = {0, 0, 0, 0};
                const int32_t b0 = v * 16;
                if ((pw == 4 || pw == 8) && !((W | off) & 3)) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int32_t b = b0 + 4 * j;
                        const int32_t row = pw == 4 ? b >> 2 : b >> 3;
                        o[j] = *reinterpret_cast<const uint32_t*>(tile + row * W + off + (b - row * pw));
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        const int32_t b = b0 + j;
                        const int32_t row = pw == 1 ? b : pw == 4 ? b >> 2 : pw == 8 ? b >> 3 : b / pw;
                        o[j >> 2] |= (uint32_t)tile[row * W + off + (b - row * pw)] << (8 * (j & 3));
                    }
                }
                *reinterpret_cast<uint4*>(dst + (int64_t)v * 16) = make_uint4(o[0], o[1], o[2], o[3]);
            }
            for (int32_t b = (full << 4) + threadIdx.x; b < nbytes; b += KEY_WG) {
                const int32_t row = b / pw;
                dst[b] = tile[row * W + off + (b - row * pw)];
            }
        }
        __syncthreads();
    }
}

// Every part one byte wide (a tuple of dictionary codes - TPC-H Q1's key): no LDS.  Sixteen rows per lane as in
// k_dict_combine: one 16-byte load per part, the bytes interleaved in registers (every index below is a compile-time
// constant once unrolled), NP 16-byte stores.  The last, partial group of rows is copied byte by byte.
constexpr int KEY_BYTES_MAX_BLOCKS = 1024;  // x 256 lanes x 16 rows = 4 Mi rows per trip of the grid-stride loop

template <int NP>
__global__ void __launch_bounds__(KEY_WG) k_key_pack_bytes(const KeyArgs A, int64_t n, uint8_t* out) {
    const int64_t ngroups = (n + 15) / 16;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t base = g * 16;
        uint8_t* dst = out + base * NP;
        if (base + 16 > n) {
            for (int64_t r = base; r < n; ++r) {
#pragma unroll
                for (int k = 0; k < NP; ++k) out[r * NP + k] = A.part[k][r];
            }
            continue;
        }
        uint32_t w[NP][4];
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const uint4 v = *reinterpret_cast<const uint4*>(A.part[k] + base);
            w[k][0] = v.x, w[k][1] = v.y, w[k][2] = v.z, w[k][3] = v.w;
        }
        uint32_t o[NP * 4];
#pragma unroll
        for (int i = 0; i < NP * 4; ++i) o[i] = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                const int b = r * NP + k;
                o[b >> 2] |= ((w[k][r >> 2] >> (8 * (r & 3))) & 0xffu) << (8 * (b & 3));
            }
        }
#pragma unroll
        for (int q = 0; q < NP; ++q)
            reinterpret_cast<uint4*>(dst)[q] = make_uint4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
    }
}

template <int NP>
void key_launch_bytes(hipStream_t stream, const KeyArgs& A, int64_t n, uint8_t* out) {
    int64_t blocks = ((n + 15) / 16 + KEY_WG - 1) / KEY_WG;
    if (blocks > KEY_BYTES_MAX_BLOCKS) blocks = KEY_BYTES_MAX_BLOCKS;
    hipLaunchKernelGGL(k_key_pack_bytes<NP>, dim3((unsigned)blocks), dim3(KEY_WG), 0, stream, A, n, out);
}

unsigned key_grid(int64_t n) {
    int64_t b = (n + HS_KEY_TILE_ROWS - 1) / HS_KEY_TILE_ROWS;
    if (b < 1) b = 1;
    if (b > HS_KEY_MAX_BLOCKS) b = HS_KEY_MAX_BLOCKS;
    return (unsigned)b;
}

// the layout both calls share: widths -> offsets, checked against `width`
int key_layout(const char* who, const int32_t* widths, int32_t n_parts, int32_t width, KeyArgs& A) {
    int32_t sum = 0;
    for (int k = 0; k < HS_KEY_MAX_PARTS; ++k) {
        A.part[k] = nullptr;
        A.width[k] = 0;
        A.off[k] = 0;
    }
    for (int k = 0; k < n_parts; ++k) {
        if (widths[k] < 1 || widths[k] > HS_KEY_MAX_WIDTH) {
            hs_set_error("%s: part %d is %d bytes wide (1..%d)", who, k, (int)widths[k], HS_KEY_MAX_WIDTH);
            return HS_E_ARG;
        }
        A.width[k] = widths[k];
        A.off[k] = sum;
        sum += widths[k];
    }
    if (sum != width || width > HS_KEY_MAX_WIDTH) {
        hs_set_error("%s: width %d, the parts add up to %d (at most %d bytes)", who, (int)width, (int)sum, HS_KEY_MAX_WIDTH);
        return HS_E_ARG;
    }
    A.n_parts = n_parts;
    A.W = width;
    return HS_OK;
}

}  // namespace

extern "C" int hs_key_pack(void* stream, const hs_col* parts, int32_t n_parts, int64_t nrows, uint8_t* out, int32_t width) {
    if (!parts || !out || nrows < 0 || n_parts < 1 || n_parts > HS_KEY_MAX_PARTS) {
        hs_set_error("hs_key_pack: bad arguments (1..%d parts, non-null buffers)", HS_KEY_MAX_PARTS);
        return HS_E_ARG;
    }
    if (hs_refuse_narrow("hs_key_pack", parts, n_parts)) return HS_E_ARG;
    int32_t widths[HS_KEY_MAX_PARTS];
    for (int k = 0; k < n_parts; ++k) {
        const hs_col& c = parts[k];
        if (!c.data) {
            hs_set_error("hs_key_pack: part %d has no data", k);
            return HS_E_ARG;
        }
        if (c.kind == HS_I32) widths[k] = 4;
        else if (c.kind == HS_I64) widths[k] = 8;
        else if (c.kind == HS_STR && c.fixed_len >= 1) widths[k] = c.fixed_len;
        else {
            hs_set_error("hs_key_pack: part %d of kind %d / fixed_len %d: INTEGER, TIMESTAMP or a fixed-length STRING", k,
                         (int)c.kind, (int)c.fixed_len);
            return HS_E_ARG;
        }
    }
    KeyArgs A;
    const int rc = key_layout("hs_key_pack", widths, n_parts, width, A);
    if (rc) return rc;
    if ((uintptr_t)out & 15) {
        hs_set_error("hs_key_pack: output must be 16-byte aligned");
        return HS_E_ARG;
    }
    for (int k = 0; k < n_parts; ++k) A.part[k] = (const uint8_t*)parts[k].data;
    if (nrows == 0) return HS_OK;  // nothing to launch
    bool bytes = n_parts >= 2;  // a tuple of single bytes, every part 16-byte aligned: interleaved in registers
    for (int k = 0; k < n_parts; ++k) bytes = bytes && widths[k] == 1 && !((uintptr_t)parts[k].data & 15);
    hipStream_t s = (hipStream_t)stream;
    if (bytes) {
        switch (n_parts) {
            case 2: key_launch_bytes<2>(s, A, nrows, out); break;
            case 3: key_launch_bytes<3>(s, A, nrows, out); break;
            case 4: key_launch_bytes<4>(s, A, nrows, out); break;
            case 5: key_launch_bytes<5>(s, A, nrows, out); break;
            case 6: key_launch_bytes<6>(s, A, nrows, out); break;
            case 7: key_launch_bytes<7>(s, A, nrows, out); break;
            default: key_launch_bytes<8>(s, A, nrows, out); break;
        }
    } else {
        hipLaunchKernelGGL(k_key_pack, dim3(key_grid(nrows)), dim3(KEY_WG), 0, s, A, nrows, out);
    }
    ROWS_CHECK_LAUNCH("hs_key_pack");
    return HS_OK;
}

extern "C" int hs_key_unpack(void* stream, const uint8_t* keys, int32_t width, int64_t nrows, const int64_t* nrows_dev,
                             const int32_t* part_widths, int32_t n_parts, void* const* outs) {
    if (!keys || !part_widths || !outs || nrows < 0 || n_parts < 1 || n_parts > HS_KEY_MAX_PARTS) {
        hs_set_error("hs_key_unpack: bad arguments (1..%d parts, non-null buffers)", HS_KEY_MAX_PARTS);
        return HS_E_ARG;
    }
    KeyArgs A;
    const int rc = key_layout("hs_key_unpack", part_widths, n_parts, width, A);
    if (rc) return rc;
    for (int k = 0; k < n_parts; ++k) {
        if (!outs[k] || ((uintptr_t)outs[k] & 15)) {
            hs_set_error("hs_key_unpack: output %d is null or not 16-byte aligned", k);
            return HS_E_ARG;
        }
        A.part[k] = (const uint8_t*)outs[k];
    }
    if (nrows == 0) return HS_OK;  // nothing to launch
    hipLaunchKernelGGL(k_key_unpack, dim3(key_grid(nrows)), dim3(KEY_WG), 0, (hipStream_t)stream, A, nrows, nrows_dev, keys);
    ROWS_CHECK_LAUNCH("hs_key_unpack");
    return HS_OK;
}
