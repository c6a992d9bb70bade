// hs_engine.hip - the stage-level C ABI: a GROUP BY query over one BlockFile table, end to end, without Python.
//
// What the reference does per query: the driver turns the physical plan into jobs, ships them to a worker process
// over stdin (src/mini_spark/execution.py:182-219, jobs.py:45-79) and the worker (zig-src/src/job.zig:3-57) reads
// BlockFile blocks (block_file.zig:225-306), runs the stage's task chain and writes shuffle / result files.  Here a
// host - the Python engine, or a cgo / JNI / FFI binding - hands over a PLAN BLOB (hs_stage_plan:
// the lowered programs of [scan -> WHERE -> partial aggregate] and [final merge -> projection -> result]) and gets the
// result columns back:
//
//   hs_engine_create -> hs_table_open (native BlockFile reader: header / footer / column spans, column pruning,
//   parallel pread into pinned staging, async H2D) -> hs_stage_prepare -> hs_stage_run -> hs_result_columns /
//   hs_result_write_blockfile.
//
// Everything that lived in minispark_amd/device.py for this path lives here too: slab and result-image layout, chunk
// geometry, workspace management, the capacity retry (a dictionary overflow grows the capacities and re-runs), the
// steady-state replay (the launches of a run are captured, hs_capture.h, and re-issued by later runs), and the
// zero-copy hand-over (result image in mapped pinned memory, "done" word polled by the host).  Queries that do not
// fit the on-chip tiers return HS_E_LIMIT: the caller takes the general operator sequence.
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "hs_device.h"

void hs_set_error(const char* fmt, ...);

namespace {

constexpr size_t kPad = 64;  // slack behind every device buffer (16-byte row-quad loads run past the last row)

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) {
        o.p = nullptr;
        o.bytes = 0;
    }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = o.p;
            bytes = o.bytes;
            o.p = nullptr;
            o.bytes = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    bool alloc(size_t n, bool zero = false) {
        release();
        if (hipMalloc(&p, n + kPad) != hipSuccess) {
            p = nullptr;
            return false;
        }
        bytes = n;
        if (zero && hipMemset(p, 0, n + kPad) != hipSuccess) return false;
        return true;
    }
};

struct Column {
    int32_t type = 0;  // BlockFile type code: 0 INTEGER, 1 STRING, 2 FLOAT, 3 TIMESTAMP (constants.py:19-22)
    std::string name;
    bool loaded = false;
    hs_col col{};
    DevBuf data, lens, offs;
};

struct Span {
    int64_t off = 0, bytes = 0;
};

}  // namespace

// Pinned staging of the reader (hs_table_load): allocated once per engine - pinning host memory costs milliseconds per
// allocation, round 2 paid 2 x 16 MiB x 8 threads of it on every load.
struct PinnedPool {
    void* base = nullptr;
    size_t slot_bytes = 0;
    int n_slots = 0;
    ~PinnedPool() {
        if (base) (void)hipHostFree(base);
    }
    bool ensure(size_t bytes_per_slot, int slots) {
        if (base && slot_bytes >= bytes_per_slot && n_slots >= slots) return true;
        if (base) (void)hipHostFree(base);
        base = nullptr;
        if (hipHostMalloc(&base, bytes_per_slot * (size_t)slots, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess) {
            base = nullptr;
            return false;
        }
        slot_bytes = bytes_per_slot;
        n_slots = slots;
        return true;
    }
    char* slot(int i) const { return (char*)base + (size_t)i * slot_bytes; }
};

struct ReaderPool;
void hs_reader_pool_free(ReaderPool* p);

struct hs_engine {
    int device = 0;
    DevBuf flags;  // one status word
    PinnedPool staging;
    ReaderPool* readers = nullptr;   // persistent reader threads (created by the first load)
    double last_load_seconds = 0.0;  // wall time of the last hs_table_load's read + copy pipeline
    int64_t last_load_bytes = 0;
    ~hs_engine() {
        if (readers) hs_reader_pool_free(readers);
    }
};

struct hs_table {
    hs_engine* engine = nullptr;
    std::string path;
    std::vector<Column> cols;
    std::vector<int64_t> block_rows;     // local blocks
    std::vector<int32_t> file_blocks;    // their global ids
    std::vector<std::vector<Span>> spans;  // [local block][column] byte span of the payload
    int32_t total_blocks = 0;
    int64_t nrows = 0;
    bool attached = false;  // columns are caller-owned device memory
};

namespace {

bool read_exact(int fd, void* dst, size_t n, int64_t off) {
    size_t done = 0;
    while (done < n) {
        const ssize_t got = pread(fd, (char*)dst + done, n - done, off + (int64_t)done);
        if (got <= 0) return false;
        done += (size_t)got;
    }
    return true;
}

int kind_of_type(int32_t type) { return type == 0 ? HS_I32 : type == 2 ? HS_F32 : type == 3 ? HS_I64 : HS_STR; }
int elem_bytes(int kind) { return kind == HS_I64 || kind == HS_F64 ? 8 : kind == HS_U8 ? 1 : 4; }

}  // namespace

extern "C" int hs_engine_create(int32_t device, hs_engine** out) {
    if (!out) {
        hs_set_error("hs_engine_create: null argument");
        return HS_E_ARG;
    }
    if (hipSetDevice(device) != hipSuccess) {
        hs_set_error("hs_engine_create: no such GPU (%d) - there is no CPU execution path", device);
        return HS_E_LAUNCH;
    }
    hs_engine* e = new hs_engine();
    e->device = device;
    if (!e->flags.alloc(16, true)) {
        delete e;
        hs_set_error("hs_engine_create: out of device memory");
        return HS_E_LAUNCH;
    }
    *out = e;
    return HS_OK;
}

extern "C" void hs_engine_destroy(hs_engine* e) { delete e; }

extern "C" int hs_engine_load_stats(const hs_engine* e, double* seconds, int64_t* bytes) {
    if (!e) {
        hs_set_error("hs_engine_load_stats: null engine");
        return HS_E_ARG;
    }
    if (seconds) *seconds = e->last_load_seconds;
    if (bytes) *bytes = e->last_load_bytes;
    return HS_OK;
}

// ---- BlockFile reader (format: SURVEY.md appendix A; reference io.py:47-170, zig block_file.zig:225-306) --------------
extern "C" int hs_table_open(hs_engine* e, const char* path, int32_t rank, int32_t world, hs_table** out) {
    if (!e || !path || !out || world < 1 || rank < 0 || rank >= world) {
        hs_set_error("hs_table_open: bad arguments");
        return HS_E_ARG;
    }
    const int fd = open(path, O_RDONLY);
    if (fd < 0) {
        hs_set_error("hs_table_open: cannot open %s", path);
        return HS_E_ARG;
    }
    struct stat st;
    fstat(fd, &st);
    const int64_t size = st.st_size;
    auto fail = [&](const char* what) {
        close(fd);
        hs_set_error("hs_table_open: %s: %s", path, what);
        return HS_E_ARG;
    };
    uint8_t ncols = 0;
    if (size < 5 || !read_exact(fd, &ncols, 1, 0)) return fail("not a BlockFile (too short)");
    hs_table* t = new hs_table();
    t->engine = e;
    t->path = path;
    int64_t pos = 1;
    for (int c = 0; c < ncols; ++c) {
        uint8_t hdr[2];
        if (!read_exact(fd, hdr, 2, pos)) {
            delete t;
            return fail("truncated header");
        }
        std::string name(hdr[1], '\0');
        if (hdr[1] && !read_exact(fd, &name[0], hdr[1], pos + 2)) {
            delete t;
            return fail("truncated header");
        }
        pos += 2 + hdr[1];
        Column col;
        col.type = hdr[0];
        col.name = name;
        if (hdr[0] > 3) {
            delete t;
            return fail("unknown column type");
        }
        t->cols.push_back(std::move(col));
    }
    uint32_t nblocks = 0;
    if (!read_exact(fd, &nblocks, 4, size - 4) || (int64_t)nblocks * 8 + 4 + pos > size) {
        delete t;
        return fail("bad footer");
    }
    std::vector<uint64_t> starts(nblocks);
    if (nblocks && !read_exact(fd, starts.data(), (size_t)nblocks * 8, size - 4 - (int64_t)nblocks * 8)) {
        delete t;
        return fail("bad footer");
    }
    t->total_blocks = (int32_t)nblocks;
    for (uint32_t b = 0; b < nblocks; ++b) {
        if ((int32_t)(b % (uint32_t)world) != rank) continue;  // block b lives on rank b % world (plan.py:90-93: independent jobs)
        uint32_t rows = 0;
        int64_t p = (int64_t)starts[b];
        if (!read_exact(fd, &rows, 4, p)) {
            delete t;
            return fail("truncated block");
        }
        p += 4;
        std::vector<Span> spans(ncols);
        for (int c = 0; c < ncols; ++c) {
            uint64_t bytes = 0;
            if (!read_exact(fd, &bytes, 8, p)) {
                delete t;
                return fail("truncated block");
            }
            spans[c] = Span{p + 8, (int64_t)bytes};
            p += 8 + (int64_t)bytes;
            const int kind = kind_of_type(t->cols[c].type);
            if ((kind != HS_STR && (int64_t)bytes != (int64_t)rows * elem_bytes(kind)) || (kind == HS_STR && (int64_t)bytes < rows) ||
                p > size) {
                delete t;
                return fail("column payload size does not match the block's row count");
            }
        }
        t->block_rows.push_back(rows);
        t->file_blocks.push_back((int32_t)b);
        t->spans.push_back(std::move(spans));
        t->nrows += rows;
    }
    close(fd);
    *out = t;
    return HS_OK;
}

extern "C" void hs_table_close(hs_table* t) { delete t; }

extern "C" int hs_table_info(const hs_table* t, int32_t* n_cols, int64_t* n_rows, int32_t* n_blocks, int32_t* total_blocks) {
    if (!t) {
        hs_set_error("hs_table_info: null table");
        return HS_E_ARG;
    }
    if (n_cols) *n_cols = (int32_t)t->cols.size();
    if (n_rows) *n_rows = t->nrows;
    if (n_blocks) *n_blocks = (int32_t)t->block_rows.size();
    if (total_blocks) *total_blocks = t->total_blocks;
    return HS_OK;
}

extern "C" int hs_table_schema(const hs_table* t, int32_t col, int32_t* type, char* name, int32_t name_cap) {
    if (!t || col < 0 || col >= (int32_t)t->cols.size()) {
        hs_set_error("hs_table_schema: no such column");
        return HS_E_ARG;
    }
    if (type) *type = t->cols[col].type;
    if (name && name_cap > 0) {
        strncpy(name, t->cols[col].name.c_str(), (size_t)name_cap - 1);
        name[name_cap - 1] = 0;
    }
    return HS_OK;
}

extern "C" int hs_table_column(const hs_table* t, int32_t col, hs_col* out, int64_t* n_rows) {
    if (!t || !out || col < 0 || col >= (int32_t)t->cols.size() || !t->cols[col].loaded) {
        hs_set_error("hs_table_column: column not loaded");
        return HS_E_ARG;
    }
    *out = t->cols[col].col;
    if (n_rows) *n_rows = t->nrows;
    return HS_OK;
}

// Caller-owned device columns as a table (synthetic data, or columns another reader placed in HBM).
extern "C" int hs_table_attach(hs_engine* e, int32_t n_cols, const hs_col* cols, const int32_t* types, const int64_t* block_rows,
                               int32_t n_blocks, hs_table** out) {
    if (!e || !cols || !types || !block_rows || !out || n_cols < 1 || n_blocks < 0) {
        hs_set_error("hs_table_attach: bad arguments");
        return HS_E_ARG;
    }
    if (hs_refuse_narrow("hs_table_attach", cols, n_cols)) return HS_E_ARG;  // (so no stage ever sees one)
    hs_table* t = new hs_table();
    t->engine = e;
    t->attached = true;
    for (int c = 0; c < n_cols; ++c) {
        Column col;
        col.type = types[c];
        col.name = "c" + std::to_string(c);
        col.col = cols[c];
        col.loaded = cols[c].data != nullptr;
        t->cols.push_back(std::move(col));
    }
    for (int b = 0; b < n_blocks; ++b) {
        t->block_rows.push_back(block_rows[b]);
        t->file_blocks.push_back(b);
        t->nrows += block_rows[b];
    }
    t->total_blocks = n_blocks;
    *out = t;
    return HS_OK;
}

namespace {

struct Piece {
    int64_t file_off, bytes;
    char* dst;  // device address
};

// Reader threads (round 3): the column spans are cut into chunks of HS_READ_CHUNK bytes; every thread owns HS_READ_SLOTS
// pinned slots of the engine's pool and a stream, claims the next chunk, preads it into a free slot (page cache ->
// pinned memory: the one host-side copy) and queues its H2D copy; a slot is reused once its copy's event has fired.
// With chunks of a few MiB, up to 16 threads and 4 slots each, the preads of all threads and the DMA of earlier
// chunks overlap from the first millisecond on (round 2: 8 threads x 2 slots of whole 8-16 MiB spans, pinned memory
// allocated per call: 27 GB/s of the link's 63).
constexpr int64_t HS_READ_CHUNK = 4ll << 20;
constexpr int HS_READ_SLOTS = 4;
constexpr int HS_READ_THREADS_MAX = 16;

int reader_threads() {
    // 8 by default: measured on the test box (16 host threads granted) 6-10 readers all reach 42-45 GB/s at sf=10,
    // 16 fall back to 37-41 (they contend for the page cache / memory bandwidth, not for the link)
    int n = 8;
    if (const char* env = getenv("HIPSPARK_INGEST_READERS")) n = atoi(env);
    const unsigned hw = std::thread::hardware_concurrency();
    if (hw && n > (int)hw) n = (int)hw;
    return n < 1 ? 1 : (n > HS_READ_THREADS_MAX ? HS_READ_THREADS_MAX : n);
}

// Host-to-device copy of one staged chunk by a KERNEL that reads the pinned slot over PCIe (the slot is mapped into
// the device's address space): 16-byte loads from host memory, 16-byte stores to HBM.  HIPSPARK_INGEST_COPY=sdma uses
// hipMemcpyAsync (the DMA engines) instead; the two measure alike (42-45 GB/s at sf=10, ~50 GB/s at sf=30).
__global__ void __launch_bounds__(256) k_pull_chunk(const uint4* __restrict__ src, uint4* __restrict__ dst, int64_t n16,
                                                    const uint8_t* __restrict__ src_tail, uint8_t* __restrict__ dst_tail, int tail) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = src[i];
    if (blockIdx.x == 0 && (int)threadIdx.x < tail) dst_tail[threadIdx.x] = src_tail[threadIdx.x];
}

bool copy_by_kernel() {
    static const bool k = !(getenv("HIPSPARK_INGEST_COPY") && getenv("HIPSPARK_INGEST_COPY")[0] == 's');
    return k;
}

}  // namespace

// The engine's reader threads live as long as the engine: a thread's first HIP call, its stream and its events cost
// milliseconds - at sf=10 (1.56 GB, ~31 ms at the link's practical rate) that was 5 ms of every load.
struct ReaderPool {
    struct Job {
        const std::string* path = nullptr;
        const std::vector<Piece>* pieces = nullptr;
        char* pool_dev = nullptr;
        bool by_kernel = false;
        std::atomic<size_t> next{0};
        std::atomic<bool> failed{false};
    };
    hs_engine* engine = nullptr;
    std::vector<std::thread> threads;
    std::mutex m;
    std::condition_variable cv_job, cv_done;
    Job* job = nullptr;
    uint64_t job_id = 0;
    int working = 0;
    bool stop = false;

    ~ReaderPool() {
        {
            std::lock_guard<std::mutex> lock(m);
            stop = true;
        }
        cv_job.notify_all();
        for (std::thread& th : threads) th.join();
    }

    // `seen0`: the id of the last job posted before this thread existed - a thread added to a pool that has already run
    // jobs must wait for the NEXT post, not wake on the stale id with `job` reset to null
    void worker(int w, uint64_t seen0) {
        const bool dev_ok = hipSetDevice(engine->device) == hipSuccess;
        hipStream_t stream = nullptr;
        hipEvent_t ev[HS_READ_SLOTS] = {};
        bool ok_setup = dev_ok && hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) == hipSuccess;
        for (int k = 0; ok_setup && k < HS_READ_SLOTS; ++k) ok_setup = hipEventCreateWithFlags(&ev[k], hipEventDisableTiming) == hipSuccess;
        uint64_t seen = seen0;
        for (;;) {
            Job* j = nullptr;
            {
                std::unique_lock<std::mutex> lock(m);
                cv_job.wait(lock, [&] { return stop || job_id != seen; });
                if (stop) break;
                seen = job_id;
                j = job;
            }
            if (!j) continue;  // (never counted in `working`: nothing to report)
            bool ok = ok_setup;
            const int fd = ok ? open(j->path->c_str(), O_RDONLY) : -1;
            ok = ok && fd >= 0;
            bool used[HS_READ_SLOTS] = {};
            const std::vector<Piece>& pieces = *j->pieces;
            for (int turn = 0; ok && !j->failed; turn = (turn + 1) % HS_READ_SLOTS) {
                const size_t i = j->next.fetch_add(1);
                if (i >= pieces.size()) break;
                const Piece& p = pieces[i];
                char* slot = engine->staging.slot(w * HS_READ_SLOTS + turn);
                if (used[turn]) ok = hipEventSynchronize(ev[turn]) == hipSuccess;  // the slot's previous copy has left it
                ok = ok && read_exact(fd, slot, (size_t)p.bytes, p.file_off);
                if (ok && j->by_kernel && (((uintptr_t)p.dst) & 15) == 0) {
                    // (a destination inside a column buffer is 16-byte aligned whenever the span starts on a multiple of
                    // 16 bytes of the column: always for the fixed-width columns of 2 Mi-row blocks)
                    char* mapped = j->pool_dev + (slot - (char*)engine->staging.base);
                    const int64_t n16 = p.bytes / 16;
                    const int tail = (int)(p.bytes - n16 * 16);
                    hipLaunchKernelGGL(k_pull_chunk, dim3(64), dim3(256), 0, stream, (const uint4*)mapped, (uint4*)p.dst, n16,
                                       (const uint8_t*)mapped + n16 * 16, (uint8_t*)p.dst + n16 * 16, tail);
                    ok = hipGetLastError() == hipSuccess;
                } else {
                    ok = ok && hipMemcpyAsync(p.dst, slot, (size_t)p.bytes, hipMemcpyHostToDevice, stream) == hipSuccess;
                }
                ok = ok && hipEventRecord(ev[turn], stream) == hipSuccess;
                used[turn] = true;
            }
            if (stream) ok = (hipStreamSynchronize(stream) == hipSuccess) && ok;
            if (fd >= 0) close(fd);
            if (!ok) j->failed = true;
            {
                std::lock_guard<std::mutex> lock(m);
                --working;
            }
            cv_done.notify_all();
        }
        for (int k = 0; k < HS_READ_SLOTS; ++k)
            if (ev[k]) (void)hipEventDestroy(ev[k]);
        if (stream) (void)hipStreamDestroy(stream);
    }

    bool run(hs_engine* e, Job& j, int n_threads) {
        engine = e;
        while ((int)threads.size() < n_threads) {
            const int w = (int)threads.size();
            const uint64_t posted = job_id;  // run() is the only writer and is not re-entered
            threads.emplace_back([this, w, posted] { worker(w, posted); });
        }
        {
            std::lock_guard<std::mutex> lock(m);
            job = &j;
            ++job_id;
            working = (int)threads.size();
        }
        cv_job.notify_all();
        std::unique_lock<std::mutex> lock(m);
        cv_done.wait(lock, [&] { return working == 0; });
        job = nullptr;
        return !j.failed;
    }
};

void hs_reader_pool_free(ReaderPool* p) { delete p; }

namespace {

bool run_pieces(hs_engine* e, const std::string& path, const std::vector<Piece>& spans, std::string& err) {
    if (spans.empty()) return true;
    std::vector<Piece> pieces;
    int64_t total = 0;
    for (const Piece& p : spans) {
        for (int64_t at = 0; at < p.bytes; at += HS_READ_CHUNK) {
            const int64_t n = p.bytes - at < HS_READ_CHUNK ? p.bytes - at : HS_READ_CHUNK;
            pieces.push_back(Piece{p.file_off + at, n, p.dst + at});
        }
        total += p.bytes;
    }
    if (!e->staging.ensure((size_t)HS_READ_CHUNK, HS_READ_THREADS_MAX * HS_READ_SLOTS)) {
        err = "cannot pin host staging memory";
        return false;
    }
    if (!e->readers) e->readers = new ReaderPool();
    ReaderPool::Job job;
    job.path = &path;
    job.pieces = &pieces;
    job.by_kernel = copy_by_kernel() && hipHostGetDevicePointer((void**)&job.pool_dev, e->staging.base, 0) == hipSuccess && job.pool_dev;
    const auto t0 = std::chrono::steady_clock::now();
    const bool ok = e->readers->run(e, job, reader_threads());
    e->last_load_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    e->last_load_bytes = total;
    if (!ok) err = "read or host-to-device copy failed";
    return ok;
}

}  // namespace

// The reader's pipeline for a caller that owns the destination buffers (the Python engine's table loader): spans of the
// file -> device addresses.  Same threads, pinned pool and chunking as hs_table_load.
extern "C" int hs_read_spans(hs_engine* e, const char* path, const hs_span* spans, int32_t n_spans) {
    if (!e || !path || n_spans < 0 || (n_spans > 0 && !spans)) {
        hs_set_error("hs_read_spans: bad arguments");
        return HS_E_ARG;
    }
    if (hipSetDevice(e->device) != hipSuccess) return HS_E_LAUNCH;
    std::vector<Piece> pieces;
    for (int i = 0; i < n_spans; ++i) {
        if (spans[i].bytes < 0 || spans[i].file_offset < 0 || (spans[i].bytes > 0 && !spans[i].dst)) {
            hs_set_error("hs_read_spans: span %d is malformed", i);
            return HS_E_ARG;
        }
        if (spans[i].bytes) pieces.push_back(Piece{spans[i].file_offset, spans[i].bytes, (char*)spans[i].dst});
    }
    std::string err;
    if (!run_pieces(e, path, pieces, err)) {
        hs_set_error("hs_read_spans: %s: %s", path, err.c_str());
        return HS_E_LAUNCH;
    }
    return HS_OK;
}

// Load the byte spans of the listed columns (column pruning: nothing else is read) into one contiguous device buffer
// per column across all local blocks; STRING columns get their offsets from a device prefix sum and fixed_len when every
// row has the same length.  Idempotent per column.
extern "C" int hs_table_load(hs_engine* e, hs_table* t, const int32_t* col_ids, int32_t n) {
    if (!e || !t || !col_ids || n < 0) {
        hs_set_error("hs_table_load: bad arguments");
        return HS_E_ARG;
    }
    if (hipSetDevice(e->device) != hipSuccess) return HS_E_LAUNCH;
    std::vector<Piece> pieces;
    std::vector<int> fresh;
    for (int k = 0; k < n; ++k) {
        const int c = col_ids[k];
        if (c < 0 || c >= (int)t->cols.size()) {
            hs_set_error("hs_table_load: no such column %d", c);
            return HS_E_ARG;
        }
        Column& col = t->cols[c];
        if (col.loaded) continue;
        if (t->attached) {
            hs_set_error("hs_table_load: column %d of an attached table has no device data", c);
            return HS_E_ARG;
        }
        const int kind = kind_of_type(col.type);
        const size_t nb = t->block_rows.size();
        bool ok = true;
        if (kind == HS_STR) {
            int64_t payload = 0;
            for (size_t b = 0; b < nb; ++b) payload += t->spans[b][c].bytes - t->block_rows[b];
            ok = col.lens.alloc((size_t)t->nrows) && col.data.alloc((size_t)payload);
            int64_t row = 0, byte = 0;
            for (size_t b = 0; ok && b < nb; ++b) {
                const Span& s = t->spans[b][c];
                const int64_t rows = t->block_rows[b];
                if (rows) pieces.push_back(Piece{s.off, rows, (char*)col.lens.p + row});
                if (s.bytes > rows) pieces.push_back(Piece{s.off + rows, s.bytes - rows, (char*)col.data.p + byte});
                row += rows;
                byte += s.bytes - rows;
            }
        } else {
            ok = col.data.alloc((size_t)t->nrows * (size_t)elem_bytes(kind));
            int64_t byte = 0;
            for (size_t b = 0; ok && b < nb; ++b) {
                const Span& s = t->spans[b][c];
                if (s.bytes) pieces.push_back(Piece{s.off, s.bytes, (char*)col.data.p + byte});
                byte += s.bytes;
            }
        }
        if (!ok) {
            hs_set_error("hs_table_load: out of device memory");
            return HS_E_LAUNCH;
        }
        fresh.push_back(c);
    }
    std::string err;
    if (!run_pieces(e, t->path, pieces, err)) {
        hs_set_error("hs_table_load: %s: %s", t->path.c_str(), err.c_str());
        return HS_E_LAUNCH;
    }
    for (int c : fresh) {
        Column& col = t->cols[c];
        const int kind = kind_of_type(col.type);
        col.col = hs_col{kind, -1, col.data.p, nullptr, nullptr};
        if (kind == HS_STR) {
            col.col.lens = (const uint8_t*)col.lens.p;
            int32_t minmax[2] = {0, 0};
            if (t->nrows > 0) {
                DevBuf ws, mm;
                if (!col.offs.alloc((size_t)(t->nrows + 1) * 8) || !ws.alloc(hs_scan_ws_bytes(t->nrows)) || !mm.alloc(8)) {
                    hs_set_error("hs_table_load: out of device memory");
                    return HS_E_LAUNCH;
                }
                const int rc = hs_str_offsets(nullptr, (const uint8_t*)col.lens.p, t->nrows, (int64_t*)col.offs.p, (int32_t*)mm.p, ws.p);
                if (rc) return rc;
                if (hipMemcpy(minmax, mm.p, 8, hipMemcpyDeviceToHost) != hipSuccess) return HS_E_LAUNCH;
            }
            if (t->nrows == 0 || minmax[0] == minmax[1]) {  // every row has the same length: no offsets needed
                col.col.fixed_len = t->nrows == 0 ? 0 : minmax[0];
                col.offs.release();
            } else {
                col.col.offs = (const int64_t*)col.offs.p;
            }
        }
        col.loaded = true;
    }
    return HS_OK;
}

// =====================================================================================================
// Stages
// =====================================================================================================
// The shared-dictionary tier's buffers from the scan's unit tables to the result image (the scan stage's tier 1 and the
// join feeding a GROUP BY share them and the code that fills them)
struct SharedBufs {
    DevBuf rep, acc, ngroups, pack_start, dense_rep, order, key, accs, mrep, macc, mgroups, mkey, prog_out, image;
};

namespace {

// slots = unit tables x slots per unit table; nf = folds of the final merge
bool shared_alloc(SharedBufs& B, int64_t slots, int64_t n_units, int n_acc, int nf, int merge_cap) {
    slots = slots > 0 ? slots : 1;
    return B.rep.alloc((size_t)slots * 8) && B.acc.alloc((size_t)slots * (size_t)(n_acc > 0 ? n_acc : 1) * 8) &&
           B.ngroups.alloc((size_t)(n_units + 1) * 4) && B.pack_start.alloc((size_t)(n_units + 1) * 8) &&
           B.dense_rep.alloc((size_t)slots * 8) && B.order.alloc((size_t)slots * 8) && B.key.alloc((size_t)slots * 8) &&
           B.accs.alloc((size_t)slots * 4 * (size_t)(n_acc > 0 ? n_acc : 1)) && B.mrep.alloc((size_t)merge_cap * 8) &&
           B.macc.alloc((size_t)merge_cap * 8 * (size_t)(nf > 0 ? nf : 1)) && B.mgroups.alloc(8) &&
           B.mkey.alloc((size_t)merge_cap * 8) && B.prog_out.alloc((size_t)merge_cap * 8 * HS_MAX_OUTS);
}

// result image of the on-chip path: header 16 bytes, then every column at a 16-byte aligned offset, cap elements each
int64_t image_layout(hs_finish_spec& fin, int key_bytes, int cap) {
    int64_t pos = 16;
    for (int o = 0; o < fin.n_out; ++o) {
        hs_finish_out& out = fin.outs[o];
        const int width = out.src == 0 ? key_bytes : (out.kind == HS_I64 ? 8 : 4);
        out.offset = pos;
        pos = (pos + (int64_t)cap * width + 15) & ~(int64_t)15;
    }
    return pos;
}

// exchange slab: [flags u32][pad][row count i64] | order key i64 x slab_rows | key column | accumulator columns (4 bytes per
// row), every part 16-byte aligned; keys in their stored kinds, packed into the 64-bit key word by the finish launch.  Returns
// the slab's bytes (= the stride from one rank's slab to the next)
int64_t slab_layout(hs_slab_desc& d, int64_t slab_rows, int32_t key_kind, int32_t key_bytes, const hs_agg_spec& spec) {
    memset(&d, 0, sizeof(d));
    d.slab_rows = slab_rows;
    int64_t pos = 16;
    d.order_off = pos;
    pos += 8 * d.slab_rows;
    pos = (pos + 15) & ~(int64_t)15;
    d.key_off = pos;
    pos += (int64_t)key_bytes * d.slab_rows;
    d.n_acc = spec.n_acc;
    for (int a = 0; a < spec.n_acc; ++a) {
        pos = (pos + 15) & ~(int64_t)15;
        d.acc_off[a] = pos;
        d.acc_kind[a] = spec.is_int[a] ? HS_I32 : HS_F32;
        pos += 4 * d.slab_rows;
    }
    d.stride = (pos + 15) & ~(int64_t)15;
    d.key_kind = key_kind;
    d.key_len = key_kind == HS_STR ? key_bytes : 0;
    return d.stride;
}

// the GROUP BY key kinds the aggregate stages take as stored, and their widths: INTEGER / FLOAT / TIMESTAMP, strings of a
// fixed length of 1, 2 or 4 bytes (they pack into the 64-bit key word).  `who` names the stage in the errors
int group_key_shape(const char* who, const hs_col& kc, int32_t& kind, int32_t& bytes) {
    if (kc.kind == HS_STR) {
        if (kc.fixed_len != 1 && kc.fixed_len != 2 && kc.fixed_len != 4) {
            hs_set_error("%s: a string GROUP BY key needs a fixed length of 1, 2 or 4 bytes on this path", who);
            return HS_E_LIMIT;
        }
        bytes = kc.fixed_len;
    } else if (kc.kind == HS_I32 || kc.kind == HS_F32 || kc.kind == HS_I64) {
        bytes = elem_bytes(kc.kind);
    } else {
        hs_set_error("%s: GROUP BY key is not a stored column kind", who);
        return HS_E_LIMIT;
    }
    kind = kc.kind;
    return HS_OK;
}

// rows before unit u, u = 0 .. n: what the geometry functions and the HBM tier take
std::vector<int64_t> rows_before(const std::vector<int64_t>& block_rows) {
    std::vector<int64_t> before(block_rows.size() + 1, 0);
    for (size_t u = 0; u < block_rows.size(); ++u) before[u + 1] = before[u] + block_rows[u];
    return before;
}

// the chunks of this geometry over the units, on the device; chunk0 (optional, host): the first chunk of every unit
int chunks_upload(const char* who, const int64_t* unit_rows, int64_t n_units, const hs_agg_geom& geom, DevBuf& chunks,
                  std::vector<int64_t>* chunk0 = nullptr) {
    std::vector<hs_chunk> host((size_t)(geom.n_chunks > 0 ? geom.n_chunks : 1));
    std::vector<int64_t> first((size_t)n_units + 1, 0);
    const int rc = hs_agg_partial_chunks(unit_rows, n_units, &geom, host.data(), first.data());
    if (rc) return rc;
    if (!chunks.alloc(host.size() * sizeof(hs_chunk)) ||
        hipMemcpy(chunks.p, host.data(), host.size() * sizeof(hs_chunk), hipMemcpyHostToDevice) != hipSuccess) {
        hs_set_error("%s: out of device / pinned memory", who);
        return HS_E_LAUNCH;
    }
    if (chunk0) *chunk0 = std::move(first);
    return HS_OK;
}

// a stage's pinned result image of image_bytes, zeroed, in place of the one it had.  dev != NULL: mapped, *dev = the address
// the finish launch writes it at
bool image_alloc(void*& host, void** dev, int64_t image_bytes) {
    if (host) (void)hipHostFree(host);
    host = nullptr;
    if (dev) *dev = nullptr;
    if (hipHostMalloc(&host, (size_t)image_bytes + kPad, dev ? hipHostMallocMapped : hipHostMallocDefault) != hipSuccess) {
        host = nullptr;
        return false;
    }
    if (dev && (hipHostGetDevicePointer(dev, host, 0) != hipSuccess || !*dev)) return false;
    memset(host, 0, (size_t)image_bytes + kPad);
    return true;
}

// The launches of one run: issued as they are on the first run with the stage's capacities, recorded on the second (the
// one that is kept), replayed from then on
template <class Launch>
int run_or_replay(void*& capture, int64_t runs, int64_t& replays, void* stream, Launch launch) {
    if (capture) {
        ++replays;
        return hs_capture_replay(capture, stream);
    }
    const bool record = runs >= 1;
    int rc = record ? hs_capture_begin() : HS_OK;
    if (!rc) rc = launch();
    if (record) {
        int32_t n_ops = 0;
        void* handle = nullptr;
        const int rc2 = hs_capture_end(&handle, &n_ops);
        if (!rc && !rc2 && n_ops > 0) capture = handle;
        else if (handle) hs_capture_free(handle);
    }
    return rc;
}

// the finish launch's hand-over through the mapped image: [flags u32][done u32][row count i64]
int wait_result(const char* who, void* image_host, int32_t merge_cap, void* stream, uint32_t* flags, int64_t* rows) {
    volatile uint32_t* done = (volatile uint32_t*)image_host + 1;
    for (int64_t spins = 0; *done == 0; ++spins) {
        if (spins > 2000000) {  // a long scan: let the runtime wait instead of this core
            if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess || *done == 0) {
                hs_set_error("%s: the finish launch did not hand its result over", who);
                return HS_E_LAUNCH;
            }
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    *flags = *(volatile uint32_t*)image_host;
    const int64_t n = *(volatile int64_t*)((char*)image_host + 8);
    *rows = n < merge_cap ? n : merge_cap;
    *done = 0;  // ready for the next launch into this image
    return HS_OK;
}

// What the shared-dictionary tier does about the flags of a run: nothing (the result stands), x4 on the capacity that was
// full (the merge holds at least as many keys as a unit table; 4096 is the on-chip tiers' cap) and run again, or - past the
// cap, or with more partial rows than the on-chip merge holds - the HBM tier where its switch is on, else HS_E_LIMIT
enum class SharedNext { done, grown, to_hbm, limit };

SharedNext shared_next(const char* who, uint32_t f, bool hbm_on, int32_t& group_cap, int32_t& merge_cap) {
    const bool unit_full = f & HS_FLAG_DICT_FULL, merge_full = f & HS_FLAG_MERGE_FULL;
    if (f & HS_FLAG_MERGE_ROWS) {
        if (hbm_on) return SharedNext::to_hbm;
        hs_set_error("%s: more partial rows than the on-chip final merge holds (the HBM tier belongs to the per-operator ABI)", who);
        return SharedNext::limit;
    }
    if (!unit_full && !merge_full) return SharedNext::done;
    if ((unit_full && group_cap >= 4096) || (merge_full && merge_cap >= 4096)) {
        if (hbm_on) return SharedNext::to_hbm;
        hs_set_error("%s: GROUP BY cardinality exceeds the on-chip tiers of this path", who);
        return SharedNext::limit;
    }
    if (unit_full) group_cap *= 4;
    if (merge_full) merge_cap *= 4;
    if (merge_cap < group_cap) merge_cap = group_cap;
    if (merge_cap > 4096) merge_cap = 4096;
    return SharedNext::grown;
}

// a stage leaves the on-chip tiers for the HBM tier: their buffers go (the HBM tier's image is sized per run)
void onchip_release(void*& image_host, size_t& image_host_cap, SharedBufs& sh, DevBuf& ws) {
    if (image_host) (void)hipHostFree(image_host);
    image_host = nullptr;
    image_host_cap = 0;
    sh = SharedBufs();
    ws.release();
}

// After hs_agg_shared filled B.rep / B.acc / B.ngroups: dense partial rows -> merge in unit order -> projection -> rounding ->
// result image on the host.  kc: the key column the scan read (key_rows rows); *flags_out / *rows_out: the run's result.
int shared_tail(hipStream_t stream, SharedBufs& B, const hs_agg_spec& spec, const hs_finish_spec& fin, const hs_program& fin_prog,
                const hs_col& kc, int key_bytes, int64_t key_rows, int64_t n_units, int unit_cap, int64_t slots, int cap,
                void* image_host, int64_t image_bytes, uint32_t* flags, uint32_t* flags_out, int64_t* rows_out) {
    const int n_acc = spec.n_acc, nf = fin.n_fold;
    // dense partial rows = the reference's shuffle-file content: accumulators in their stored kinds, unit of every row
    void* acc_ptrs[HS_MAX_ACC] = {};
    int32_t acc_kinds[HS_MAX_ACC] = {};
    for (int a = 0; a < n_acc; ++a) {
        acc_ptrs[a] = (char*)B.accs.p + (size_t)a * (size_t)slots * 4;
        acc_kinds[a] = spec.is_int[a] ? HS_I32 : HS_F32;
    }
    int rc = hs_agg_pack(stream, (const int64_t*)B.rep.p, (const uint64_t*)B.acc.p, (const int32_t*)B.ngroups.p, n_units, unit_cap,
                         &spec, (int64_t*)B.pack_start.p, (int64_t*)B.dense_rep.p, acc_ptrs, acc_kinds, nullptr, (int64_t*)B.order.p);
    if (rc) return rc;
    const int64_t* n_dense = (const int64_t*)B.pack_start.p + n_units;
    rc = hs_gather_fixed(stream, kc.data, key_bytes, key_rows, (const int64_t*)B.dense_rep.p, slots, n_dense, B.key.p, flags);
    if (rc) return rc;
    // final merge (tasks.py:290-292): fold j = fold_op[j] over the dense accumulator column fold_src[j], partials in unit order
    hs_col key_dense{kc.kind, kc.kind == HS_STR ? kc.fixed_len : -1, B.key.p, nullptr, nullptr};
    hs_col fold_cols[HS_MAX_ACC];
    hs_agg_spec mspec{};
    mspec.n_acc = nf;
    for (int j = 0; j < nf; ++j) {
        const int src = fin.fold_src[j];
        fold_cols[j] = hs_col{acc_kinds[src], -1, acc_ptrs[src], nullptr, nullptr};
        mspec.op[j] = (uint8_t)fin.fold_op[j];
        mspec.is_int[j] = spec.is_int[src];
    }
    rc = hs_agg_merge(stream, &key_dense, fold_cols, &mspec, (const int64_t*)B.order.p, n_units, slots, n_dense, cap,
                      (int64_t*)B.mrep.p, (uint64_t*)B.macc.p, (int64_t*)B.mgroups.p, flags);
    if (rc) return rc;  // HS_E_LIMIT: more partial rows than the on-chip merge holds
    const int64_t* ng = (const int64_t*)B.mgroups.p;
    rc = hs_gather_fixed(stream, B.key.p, key_bytes, slots, (const int64_t*)B.mrep.p, cap, ng, B.mkey.p, flags);
    if (rc) return rc;
    // projection after the merge (AVG = sum / count ...): the merged cells are its columns (slot -> key / fold j)
    int n_prog_out = 0;
    for (int o = 0; o < fin.n_out; ++o)
        if (fin.outs[o].src == 2 && fin.outs[o].index + 1 > n_prog_out) n_prog_out = fin.outs[o].index + 1;
    int32_t prog_kinds[HS_MAX_OUTS] = {};
    if (n_prog_out > 0) {
        hs_col pcols[HS_MAX_COLS];
        for (int i = 0; i < HS_MAX_COLS; ++i) {
            const int j = fin.prog_src[i];
            if (j >= 0 && j < nf) pcols[i] = hs_col{mspec.is_int[j] ? HS_I64 : HS_F64, -1, (char*)B.macc.p + (size_t)j * (size_t)cap * 8, nullptr, nullptr};
            else pcols[i] = hs_col{kc.kind == HS_STR ? HS_U8 : kc.kind, -1, B.mkey.p, nullptr, nullptr};
        }
        void* outs[HS_MAX_OUTS] = {};
        for (int o = 0; o < fin.n_out; ++o) {
            const hs_finish_out& d = fin.outs[o];
            if (d.src == 2) prog_kinds[d.index] = d.kind == HS_F32 ? HS_F64 : HS_I64;
        }
        for (int k = 0; k < n_prog_out; ++k) outs[k] = (char*)B.prog_out.p + (size_t)k * (size_t)cap * 8;
        rc = hs_eval(stream, pcols, HS_MAX_COLS, &fin_prog, nullptr, cap, ng, outs, prog_kinds, n_prog_out, flags);
        if (rc) return rc;
    }
    // result columns in their stored kinds, at the image's offsets
    for (int o = 0; o < fin.n_out; ++o) {
        const hs_finish_out& d = fin.outs[o];
        char* dst = (char*)B.image.p + d.offset;
        if (d.src == 0) {
            if (hipMemcpyAsync(dst, B.mkey.p, (size_t)cap * (size_t)key_bytes, hipMemcpyDeviceToDevice, stream) != hipSuccess) return HS_E_LAUNCH;
            continue;
        }
        const void* cells = d.src == 1 ? (const char*)B.macc.p + (size_t)d.index * (size_t)cap * 8
                                       : (const char*)B.prog_out.p + (size_t)d.index * (size_t)cap * 8;
        const bool is_int = d.src == 1 ? mspec.is_int[d.index] != 0 : prog_kinds[d.index] == HS_I64;
        if (d.kind == HS_I64) {
            if (hipMemcpyAsync(dst, cells, (size_t)cap * 8, hipMemcpyDeviceToDevice, stream) != hipSuccess) return HS_E_LAUNCH;
        } else {
            rc = hs_quantise(stream, cells, is_int ? HS_I64 : HS_F64, cap, ng, dst, flags);
            if (rc) return rc;
        }
    }
    int64_t n_groups = 0;
    uint32_t f = 0;
    if (hipMemcpyAsync((char*)image_host, B.image.p, (size_t)image_bytes, hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipMemcpyAsync(&n_groups, ng, 8, hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipMemcpyAsync(&f, flags, 4, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
        return HS_E_LAUNCH;
    *flags_out = f;
    *rows_out = n_groups < cap ? n_groups : cap;
    return HS_OK;
}


// ---- the HBM (radix) tier's tail, shared by the scan stage and the join feeding a GROUP BY ------------------------------------
// What device.py's aggregate_partial_global / aggregate_merge_global issue per operator, behind the stage boundary: row-forming
// pass -> radix partial aggregate over the units (quantised: the shuffle-file rows, in unit order) -> radix merge of the
// partial rows as one unit -> projection -> rounding -> result image sized from the real group count, one copy to the host.
constexpr int64_t kResultBlockRows = 2 * 1024 * 1024;  // ROWS_PER_BLOCK of a result file (constants.py)

struct HbmBufs {
    DevBuf units, rows_ws, key, vals[HS_MAX_ACC], bounds, ws, status, pkey, pacc[HS_MAX_ACC], one_unit, mkey, macc, prog_out, image;
    int64_t partial_rows = 0, result_rows = 0;
};

bool hbm_grow(DevBuf& b, size_t bytes) { return b.bytes >= bytes && b.p ? true : b.alloc(bytes > 0 ? bytes : 16); }

// group counts [n_units + 1] and the radix run's status word behind them, in ONE read-back.  HS_FLAG_DICT_FULL -> HS_E_LIMIT.
int hbm_radix(hipStream_t stream, HbmBufs& H, const char* who, int32_t key_code, const hs_col& key, int64_t n, int32_t n_units,
              int64_t max_unit_rows, const int64_t* bounds_dev, const hs_col* vcols, const int32_t* vkinds, const uint64_t* cells,
              const hs_agg_spec& spec, int quantise, hs_radix_plan& plan, std::vector<int64_t>& groups, uint32_t& extra_flags) {
    int rc = hs_group_radix_plan(key_code, n, n_units, max_unit_rows > 0 ? max_unit_rows : 1, vkinds, &spec, quantise, &plan);
    if (rc == HS_E_LIMIT) {
        std::string why = hs_last_error();
        hs_set_error("%s: the radix tier does not move this key / aggregate shape (%s)", who, why.c_str());
    }
    if (rc) return rc;
    if (!hbm_grow(H.ws, hs_group_radix_ws_bytes(&plan)) || !hbm_grow(H.status, (size_t)(n_units + 2) * 8)) {
        hs_set_error("%s: out of device memory for the radix tier (%zu bytes of workspace)", who, hs_group_radix_ws_bytes(&plan));
        return HS_E_LAUNCH;
    }
    if (hipMemsetAsync(H.status.p, 0, (size_t)(n_units + 2) * 8, stream) != hipSuccess) return HS_E_LAUNCH;
    int64_t* unit_groups = (int64_t*)H.status.p;
    rc = hs_group_radix_run(stream, &plan, &key, nullptr, 0, bounds_dev, vcols, cells, &spec, H.ws.p, unit_groups,
                            (uint32_t*)(unit_groups + n_units + 1));
    if (rc == HS_E_LIMIT) {
        std::string why = hs_last_error();
        hs_set_error("%s: the radix tier does not move this key / aggregate shape (%s)", who, why.c_str());
    }
    if (rc) return rc;
    groups.assign((size_t)n_units + 2, 0);
    if (hipMemcpyAsync(groups.data(), H.status.p, (size_t)(n_units + 2) * 8, hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess) {
        hs_set_error("%s: the radix run failed (%s)", who, hipGetErrorString(hipGetLastError()));
        return HS_E_LAUNCH;
    }
    const uint32_t f = (uint32_t)groups[(size_t)n_units + 1];
    if (f & HS_FLAG_DICT_FULL) {
        hs_set_error("%s: a radix partition outgrew its dictionary (the hash-table tier belongs to the per-operator ABI)", who);
        return HS_E_LIMIT;
    }
    extra_flags |= f;
    return HS_OK;
}

// fin: the stage's copy of the plan's finish description (its offsets are rewritten for this run's group count);
// image_host / image_cap: the pinned result buffer the stage owns, re-grown as needed.
int hbm_tail(hipStream_t stream, HbmBufs& H, const char* who, const hs_col* cols, int32_t n_cols, int32_t key_slot, const hs_program& prog,
             const hs_agg_spec& spec, const std::vector<int64_t>& unit_rows, int64_t n_rows, hs_finish_spec& fin, const hs_program& fin_prog,
             int key_bytes, void*& image_host, size_t& image_cap, uint32_t* flags, uint32_t* flags_out, int64_t* rows_out) {
    const int32_t n_units = (int32_t)unit_rows.size() - 1;
    const int n_acc = spec.n_acc, nf = fin.n_fold;
    H.partial_rows = H.result_rows = 0;
    *rows_out = 0;
    uint32_t extra = 0;
    auto finish_empty = [&]() -> int {  // no rows: only the flags travel
        uint32_t f = 0;
        // (the engine's status word goes back to zero: the per-lane tier of another stage on this engine ORs into it as found)
        if (hipMemcpyAsync(&f, flags, 4, hipMemcpyDeviceToHost, stream) != hipSuccess || hipMemsetAsync(flags, 0, 4, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess)
            return HS_E_LAUNCH;
        *flags_out = f | extra;
        return HS_OK;
    };
    int32_t vk[HS_MAX_ACC] = {}, vslot[HS_MAX_ACC] = {}, n_filters = 0;
    uint64_t cells[HS_MAX_ACC] = {};
    // a program or column shape the row-forming pass refuses (a stage can get here from a shape refusal of the shared tier,
    // not only from cardinality) is a refusal of this tier: HS_E_LIMIT, and the text names it
    auto refused = [&](int rc_) -> int {
        if (rc_ == HS_E_ARG || rc_ == HS_E_LIMIT) {
            const std::string why = hs_last_error();
            hs_set_error("%s: the radix tier's row-forming pass does not take this program (%s)", who, why.c_str());
            return HS_E_LIMIT;
        }
        return rc_;
    };
    int rc = hs_agg_rows_classify(cols, n_cols, key_slot, &prog, &spec, vk, vslot, cells, &n_filters);
    if (rc) return refused(rc);
    if (n_units < 1 || n_rows == 0) return finish_empty();
    const hs_col& kc = cols[key_slot];
    const int32_t key_code = kc.kind == HS_STR ? HS_STR + 256 * kc.fixed_len : kc.kind;
    // 1. the row-forming pass: without a WHERE only the computed arguments are written (the table's own columns travel)
    bool ok = hbm_grow(H.units, (size_t)(n_units + 1) * 8) && hbm_grow(H.bounds, (size_t)(n_units + 1) * 8);
    ok = ok && hipMemcpyAsync(H.units.p, unit_rows.data(), (size_t)(n_units + 1) * 8, hipMemcpyHostToDevice, stream) == hipSuccess;
    void* out_vals[HS_MAX_ACC] = {};
    bool any_cell = false;
    for (int a = 0; a < n_acc && ok; ++a) {
        const bool stored = vk[a] >= 0 && vslot[a] >= 0;
        if (vk[a] < 0 || (stored && !n_filters)) continue;
        ok = hbm_grow(H.vals[a], (size_t)n_rows * (size_t)elem_bytes(vk[a]));
        out_vals[a] = H.vals[a].p;
        any_cell = any_cell || !stored;
    }
    if (n_filters) ok = ok && hbm_grow(H.key, (size_t)n_rows * (size_t)key_bytes);
    if (!ok) {
        hs_set_error("%s: out of device memory for the row-forming pass", who);
        return HS_E_LAUNCH;
    }
    std::vector<int64_t> pos(unit_rows);  // unit boundaries as positions
    if (n_filters || any_cell) {
        if (!hbm_grow(H.rows_ws, hs_agg_rows_ws_bytes(n_rows, n_units))) return HS_E_LAUNCH;
        rc = hs_agg_rows(stream, cols, n_cols, key_slot, &prog, &spec, (const int64_t*)H.units.p, n_units, n_rows, n_filters ? H.key.p : nullptr,
                         out_vals, vk, (int64_t*)H.bounds.p, H.rows_ws.p, flags);
        if (rc) return refused(rc);
    }
    if (n_filters) {
        if (hipMemcpyAsync(pos.data(), H.bounds.p, (size_t)(n_units + 1) * 8, hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess) {
            hs_set_error("%s: the row-forming pass failed (%s)", who, hipGetErrorString(hipGetLastError()));
            return HS_E_LAUNCH;
        }
    }
    const int64_t n = pos[(size_t)n_units];
    if (n == 0) return finish_empty();
    int64_t biggest = 1;
    for (int32_t u = 0; u < n_units; ++u) biggest = std::max(biggest, pos[(size_t)u + 1] - pos[(size_t)u]);
    // 2. partial aggregate per unit, rounded to what a shuffle file holds
    const hs_col key = n_filters ? hs_col{kc.kind, kc.kind == HS_STR ? kc.fixed_len : -1, H.key.p, nullptr, nullptr} : kc;
    hs_col vcols[HS_MAX_ACC];
    for (int a = 0; a < n_acc; ++a) {
        if (vk[a] < 0) vcols[a] = hs_col{HS_U8, -1, nullptr, nullptr, nullptr};
        else if (out_vals[a]) vcols[a] = hs_col{vk[a], -1, out_vals[a], nullptr, nullptr};
        else vcols[a] = cols[vslot[a]];
    }
    hs_radix_plan plan;
    std::vector<int64_t> groups;
    rc = hbm_radix(stream, H, who, key_code, key, n, n_units, biggest, n_filters ? (const int64_t*)H.bounds.p : (const int64_t*)H.units.p,
                   vcols, vk, cells, spec, 1, plan, groups, extra);
    if (rc) return rc;
    const int64_t np = groups[(size_t)n_units];
    H.partial_rows = np;
    if (np <= 0) return finish_empty();
    ok = hbm_grow(H.pkey, (size_t)np * (size_t)key_bytes);
    void* pacc[HS_MAX_ACC] = {};
    for (int a = 0; a < n_acc && ok; ++a) {
        ok = hbm_grow(H.pacc[a], (size_t)np * 4);
        pacc[a] = H.pacc[a].p;
    }
    if (!ok) {
        hs_set_error("%s: out of device memory for %lld partial rows", who, (long long)np);
        return HS_E_LAUNCH;
    }
    rc = hs_group_radix_emit(stream, &plan, H.ws.p, H.pkey.p, pacc);
    if (rc) return rc;
    // 3. final merge (tasks.py:290-292): the partial rows, already in merge order on one GPU, as ONE unit
    hs_agg_spec mspec{};
    mspec.n_acc = nf;
    hs_col fold_cols[HS_MAX_ACC];
    int32_t fold_kinds[HS_MAX_ACC] = {};
    uint64_t zero_cells[HS_MAX_ACC] = {};
    for (int j = 0; j < nf; ++j) {
        const int src = fin.fold_src[j];
        fold_kinds[j] = spec.is_int[src] ? HS_I32 : HS_F32;
        fold_cols[j] = hs_col{fold_kinds[j], -1, pacc[src], nullptr, nullptr};
        mspec.op[j] = (uint8_t)fin.fold_op[j];
        mspec.is_int[j] = spec.is_int[src];
    }
    const int64_t one_unit[2] = {0, np};
    if (!hbm_grow(H.one_unit, 16) || hipMemcpyAsync(H.one_unit.p, one_unit, 16, hipMemcpyHostToDevice, stream) != hipSuccess) return HS_E_LAUNCH;
    const hs_col pkey{kc.kind, kc.kind == HS_STR ? kc.fixed_len : -1, H.pkey.p, nullptr, nullptr};
    hs_radix_plan mplan;
    rc = hbm_radix(stream, H, who, key_code, pkey, np, 1, np, (const int64_t*)H.one_unit.p, fold_cols, fold_kinds, zero_cells, mspec, 0, mplan,
                   groups, extra);
    if (rc) return rc;
    const int64_t ng = groups[1];
    if (ng <= 0) return finish_empty();
    const int64_t cap = ng;
    ok = hbm_grow(H.mkey, (size_t)ng * (size_t)key_bytes) && hbm_grow(H.macc, (size_t)ng * 8 * (size_t)(nf > 0 ? nf : 1));
    if (!ok) {
        hs_set_error("%s: out of device memory for %lld result rows", who, (long long)ng);
        return HS_E_LAUNCH;
    }
    void* macc[HS_MAX_ACC] = {};
    for (int j = 0; j < nf; ++j) macc[j] = (char*)H.macc.p + (size_t)j * (size_t)cap * 8;
    rc = hs_group_radix_emit(stream, &mplan, H.ws.p, H.mkey.p, macc);
    if (rc) return rc;
    // 4. projection after the merge and rounding to the stored kinds: what shared_tail issues, over the real group count
    int n_prog_out = 0;
    for (int o = 0; o < fin.n_out; ++o)
        if (fin.outs[o].src == 2 && fin.outs[o].index + 1 > n_prog_out) n_prog_out = fin.outs[o].index + 1;
    int32_t prog_kinds[HS_MAX_OUTS] = {};
    if (n_prog_out > 0) {
        if (!hbm_grow(H.prog_out, (size_t)cap * 8 * (size_t)n_prog_out)) return HS_E_LAUNCH;
        hs_col pcols[HS_MAX_COLS];
        for (int i = 0; i < HS_MAX_COLS; ++i) {
            const int j = fin.prog_src[i];
            if (j >= 0 && j < nf) pcols[i] = hs_col{mspec.is_int[j] ? HS_I64 : HS_F64, -1, macc[j], nullptr, nullptr};
            else pcols[i] = hs_col{kc.kind == HS_STR ? HS_U8 : kc.kind, -1, H.mkey.p, nullptr, nullptr};
        }
        void* outs[HS_MAX_OUTS] = {};
        for (int o = 0; o < fin.n_out; ++o) {
            const hs_finish_out& d = fin.outs[o];
            if (d.src == 2) prog_kinds[d.index] = d.kind == HS_F32 ? HS_F64 : HS_I64;
        }
        for (int k = 0; k < n_prog_out; ++k) outs[k] = (char*)H.prog_out.p + (size_t)k * (size_t)cap * 8;
        rc = hs_eval(stream, pcols, HS_MAX_COLS, &fin_prog, nullptr, cap, nullptr, outs, prog_kinds, n_prog_out, flags);
        if (rc) return rc;
    }
    // 5. result image: header (the flags word), then every column at its offset, ng elements each; ONE copy to the host
    const int64_t image_bytes = image_layout(fin, key_bytes, (int)cap);
    if (!hbm_grow(H.image, (size_t)image_bytes)) return HS_E_LAUNCH;
    if (image_cap < (size_t)image_bytes + kPad || !image_host) {
        if (image_host) (void)hipHostFree(image_host);
        image_host = nullptr;
        image_cap = 0;
        const size_t want = (size_t)image_bytes + (size_t)image_bytes / 4 + kPad;
        if (hipHostMalloc(&image_host, want, hipHostMallocDefault) != hipSuccess) {
            image_host = nullptr;
            hs_set_error("%s: out of pinned memory for %lld result rows", who, (long long)ng);
            return HS_E_LAUNCH;
        }
        image_cap = want;
    }
    for (int o = 0; o < fin.n_out; ++o) {
        const hs_finish_out& d = fin.outs[o];
        char* dst = (char*)H.image.p + d.offset;
        if (d.src == 0) {
            if (hipMemcpyAsync(dst, H.mkey.p, (size_t)cap * (size_t)key_bytes, hipMemcpyDeviceToDevice, stream) != hipSuccess) return HS_E_LAUNCH;
            continue;
        }
        const void* src = d.src == 1 ? (const char*)macc[d.index] : (const char*)H.prog_out.p + (size_t)d.index * (size_t)cap * 8;
        const bool is_int = d.src == 1 ? mspec.is_int[d.index] != 0 : prog_kinds[d.index] == HS_I64;
        if (d.kind == HS_I64) {
            if (hipMemcpyAsync(dst, src, (size_t)cap * 8, hipMemcpyDeviceToDevice, stream) != hipSuccess) return HS_E_LAUNCH;
        } else {
            rc = hs_quantise(stream, src, is_int ? HS_I64 : HS_F64, cap, nullptr, dst, flags);
            if (rc) return rc;
        }
    }
    if (hipMemcpyAsync(H.image.p, flags, 4, hipMemcpyDeviceToDevice, stream) != hipSuccess || hipMemsetAsync(flags, 0, 4, stream) != hipSuccess ||
        hipMemcpyAsync(image_host, H.image.p, (size_t)image_bytes, hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess) {
        hs_set_error("%s: the HBM tier's tail failed (%s)", who, hipGetErrorString(hipGetLastError()));
        return HS_E_LAUNCH;
    }
    *flags_out = *(const uint32_t*)image_host | extra;
    *rows_out = ng;
    H.result_rows = ng;
    return HS_OK;
}

// ---- result files: the BlockFile format (reference io.py:47-109), written from a result image or from host columns ----------
// schema header: column count, then type code, name length and name of every column.  NULL (error set): the file cannot be made
FILE* blockfile_begin(const char* who, const char* path, int n_out, const int32_t* out_types, const char (*out_names)[64]) {
    FILE* f = fopen(path, "wb");
    if (!f) {
        hs_set_error("%s: cannot create %s", who, path);
        return nullptr;
    }
    const uint8_t nc = (uint8_t)n_out;
    fwrite(&nc, 1, 1, f);
    for (int o = 0; o < n_out; ++o) {
        const uint8_t type = (uint8_t)out_types[o];
        const uint8_t len = (uint8_t)strnlen(out_names[o], 64);
        fwrite(&type, 1, 1, f);
        fwrite(&len, 1, 1, f);
        fwrite(out_names[o], 1, len, f);
    }
    return f;
}

// footer: where every block starts, the block count; false when the file did not take every byte written since blockfile_begin
bool blockfile_end(FILE* f, const std::vector<uint64_t>& starts) {
    fwrite(starts.data(), 8, starts.size(), f);
    const uint32_t nblocks = (uint32_t)starts.size();
    fwrite(&nblocks, 4, 1, f);
    return fclose(f) == 0;
}

// A result image as a BlockFile (tasks.py:400-410): one block for the on-chip path (rows_per_block 0), blocks of
// rows_per_block rows for the HBM tier; a key of dictionary codes (dict != NULL) is decoded through the dictionary.  `who`
// names the entry point in errors.
int write_image_blockfile(const char* who, const char* path, const hs_finish_spec& fin, const int32_t* out_types,
                          const char (*out_names)[64], const void* image_host, int64_t last_rows, int key_kind, int key_bytes,
                          const std::vector<std::string>* dict, int64_t rows_per_block = 0) {
    if (last_rows == 0) return HS_OK;  // empty result: the reference writes no file (tasks.py:405)
    const int n_out = fin.n_out;
    FILE* f = blockfile_begin(who, path, n_out, out_types, out_names);
    if (!f) return HS_E_ARG;
    if (rows_per_block < 1) rows_per_block = last_rows;
    std::vector<uint64_t> starts;
    bool ok = true;
    for (int64_t lo = 0; lo < last_rows; lo += rows_per_block) {  // a result larger than a block continues in further blocks
        const uint32_t rows = (uint32_t)(lo + rows_per_block < last_rows ? rows_per_block : last_rows - lo);
        starts.push_back((uint64_t)ftell(f));
        fwrite(&rows, 4, 1, f);
        for (int o = 0; o < n_out; ++o) {
            const hs_finish_out& d = fin.outs[o];
            const int width = d.src == 0 ? key_bytes : (d.kind == HS_I64 ? 8 : 4);
            const uint8_t* col = (const uint8_t*)image_host + d.offset + (size_t)lo * (size_t)width;
            if (d.src == 0 && dict) {  // code bytes -> the strings they stand for
                uint64_t bytes = rows;
                for (uint32_t r = 0; r < rows; ++r) {
                    if (col[r] >= dict->size()) ok = false;
                    else bytes += (*dict)[col[r]].size();
                }
                fwrite(&bytes, 8, 1, f);
                for (uint32_t r = 0; ok && r < rows; ++r) {
                    const uint8_t len = (uint8_t)(*dict)[col[r]].size();
                    fwrite(&len, 1, 1, f);
                }
                for (uint32_t r = 0; ok && r < rows; ++r) fwrite((*dict)[col[r]].data(), 1, (*dict)[col[r]].size(), f);
                continue;
            }
            const bool is_key_string = d.src == 0 && key_kind == HS_STR;
            const uint64_t bytes = (uint64_t)rows * (uint64_t)width + (is_key_string ? rows : 0);
            fwrite(&bytes, 8, 1, f);
            if (is_key_string) {  // STRING payload: the length bytes, then the strings
                const std::vector<uint8_t> lens(rows, (uint8_t)width);
                fwrite(lens.data(), 1, rows, f);
            }
            fwrite(col, 1, (size_t)rows * (size_t)width, f);
        }
    }
    ok = blockfile_end(f, starts) && ok;
    if (!ok) {
        hs_set_error("%s: write to %s failed (or a key code outside the dictionary)", who, path);
        return HS_E_ARG;
    }
    return HS_OK;
}

struct HostCol {  // one result column on the host: fixed-width values, or lens + payload (width -1)
    std::vector<uint8_t> data, lens;
    int width = 0;
};

// Host columns as a BlockFile of rows_per_block-row blocks (reference tasks.py:391-410 + io.py:217-252: a result larger
// than a block continues in further blocks; an empty result writes no file).
int write_rows_blockfile(const char* who, const char* path, int n_out, const int32_t* out_types, const char (*out_names)[64],
                         const std::vector<HostCol>& outs, int64_t last_rows, int64_t rows_per_block) {
    if (last_rows == 0) return HS_OK;
    FILE* f = blockfile_begin(who, path, n_out, out_types, out_names);
    if (!f) return HS_E_ARG;
    std::vector<uint64_t> starts;
    std::vector<int64_t> str_pos((size_t)n_out, 0);  // byte position inside a string column's payload
    for (int64_t lo = 0; lo < last_rows; lo += rows_per_block) {
        const int64_t hi = lo + rows_per_block < last_rows ? lo + rows_per_block : last_rows;
        const uint32_t rows = (uint32_t)(hi - lo);
        starts.push_back((uint64_t)ftell(f));
        fwrite(&rows, 4, 1, f);
        for (int o = 0; o < n_out; ++o) {
            const HostCol& out = outs[(size_t)o];
            if (out.width > 0) {
                const uint64_t bytes = (uint64_t)rows * (uint64_t)out.width;
                fwrite(&bytes, 8, 1, f);
                fwrite(out.data.data() + (size_t)lo * (size_t)out.width, 1, (size_t)bytes, f);
            } else {
                uint64_t payload = 0;
                for (int64_t r = lo; r < hi; ++r) payload += out.lens[(size_t)r];
                const uint64_t bytes = rows + payload;
                fwrite(&bytes, 8, 1, f);
                fwrite(out.lens.data() + lo, 1, rows, f);
                fwrite(out.data.data() + str_pos[(size_t)o], 1, (size_t)payload, f);
                str_pos[(size_t)o] += (int64_t)payload;
            }
        }
    }
    if (!blockfile_end(f, starts)) {
        hs_set_error("%s: write to %s failed", who, path);
        return HS_E_ARG;
    }
    return HS_OK;
}

}  // namespace

struct hs_stage {
    hs_engine* engine = nullptr;
    hs_table* table = nullptr;
    hs_stage_plan plan{};
    int32_t group_cap = 4, merge_cap = 16;
    int32_t world = 1, n_order = 1;
    // prepared state (rebuilt when a capacity grows)
    bool ready = false;
    hs_col cols[HS_MAX_COLS];
    hs_agg_geom geom{};
    hs_slab_desc desc{};
    hs_finish_spec fin{};
    int32_t key_bytes = 0;
    int64_t n_units = 0, slab_bytes = 0, image_bytes = 0;
    DevBuf chunks, chunk0, unit_ids, slab, ws, scratch;
    // round 3: tens to thousands of groups per block - the shared-dictionary tier + the general operator sequence after it
    // (pack -> key gather -> merge -> key gather / projection -> rounding), all behind hs_stage_run
    int32_t tier = 0;  // 0: per-lane tables + the one-launch finish; 1: shared dictionary + general tail; 2: HBM (radix) tier
    DevBuf key_col, key_wide;  // a computed GROUP BY key (plan version 2): the 4-byte column the scan reads + its i64 evaluation
    hs_col kcols[HS_MAX_COLS];
    SharedBufs sh;
    int64_t sh_slots = 0;
    void* image_host = nullptr;  // pinned, mapped
    void* image_dev = nullptr;
    void* capture = nullptr;     // steady state: the launches of one run
    int64_t runs = 0, replays = 0, grows = 0;
    // the HBM (radix) tier (tier 2), taken past the on-chip tiers when the stage's switch is on
    bool hbm_on = false;
    HbmBufs hbm;
    size_t image_host_cap = 0;
    std::vector<int64_t> unit_rows;
    int32_t last_tier = 0;
    int64_t tier_switches = 0;
    // last result
    uint32_t last_flags = 0;
    int64_t last_rows = 0;
    ~hs_stage() {
        if (capture) hs_capture_free(capture);
        if (image_host) (void)hipHostFree(image_host);
    }
};

namespace {

// program slots -> the table's columns; a computed key (plan version 2) gets its own 4-byte column next to them
int bind_columns(hs_stage* s) {
    hs_table* t = s->table;
    const hs_stage_plan& P = s->plan;
    for (int i = 0; i < P.n_cols; ++i)
        if (i != P.key_slot || !P.key_computed) s->cols[i] = t->cols[P.col_ids[i]].col;
    if (!P.key_computed) return HS_OK;
    for (int i = 0; i < P.n_kcols; ++i) s->kcols[i] = t->cols[P.kcol_ids[i]].col;
    const size_t rows = (size_t)(t->nrows > 0 ? t->nrows : 1);
    if (!s->key_col.p && !(s->key_col.alloc(rows * 4 + kPad, true) && s->key_wide.alloc(rows * 8 + kPad))) {
        hs_set_error("hs_stage: out of device memory for the computed key column");
        return HS_E_LAUNCH;
    }
    s->cols[P.key_slot] = hs_col{HS_I32, -1, s->key_col.p, nullptr, nullptr};
    return HS_OK;
}

// ProjectTask in front of the aggregate (reference tasks.py:32-35), for the key column alone: one evaluation per run
int compute_key(hs_stage* s, void* stream) {
    const hs_stage_plan& P = s->plan;
    if (!P.key_computed || s->table->nrows == 0) return HS_OK;
    void* outs[1] = {s->key_wide.p};
    const int32_t kinds[1] = {HS_I64};
    uint32_t* flags = (uint32_t*)s->engine->flags.p;
    int rc = hs_eval(stream, s->kcols, P.n_kcols, &P.key_prog, nullptr, s->table->nrows, nullptr, outs, kinds, 1, flags);
    if (!rc) rc = hs_quantise(stream, s->key_wide.p, HS_I64, s->table->nrows, nullptr, s->key_col.p, flags);
    return rc;
}

int stage_prepare(hs_stage* s) {
    hs_table* t = s->table;
    const hs_stage_plan& P = s->plan;
    if (s->capture) {
        hs_capture_free(s->capture);
        s->capture = nullptr;
    }
    s->ready = false;
    if (const int rc0 = bind_columns(s)) return rc0;
    const hs_col& kc = s->cols[P.key_slot];
    int32_t key_kind = 0;
    if (const int rck = group_key_shape("hs_stage", kc, key_kind, s->key_bytes)) return rck;
    // units = the table's local blocks (reference: one ScanJob per block, plan.py:90-93)
    int rc = hs_agg_partial_geom(s->unit_rows.data(), s->n_units, P.spec.n_acc, s->group_cap, &s->geom);
    if (rc) return rc;  // HS_E_LIMIT: the private-table tier does not hold this query
    std::vector<int64_t> chunk0;
    rc = chunks_upload("hs_stage", s->unit_rows.data(), s->n_units, s->geom, s->chunks, &chunk0);
    if (rc) return rc;
    std::vector<int64_t> ids(t->file_blocks.begin(), t->file_blocks.end());
    bool ok = s->chunk0.alloc(chunk0.size() * 8) && s->unit_ids.alloc((ids.size() ? ids.size() : 1) * 8) && s->ws.alloc(s->geom.ws_bytes, true);
    ok = ok && hipMemcpy(s->chunk0.p, chunk0.data(), chunk0.size() * 8, hipMemcpyHostToDevice) == hipSuccess &&
         (ids.empty() || hipMemcpy(s->unit_ids.p, ids.data(), ids.size() * 8, hipMemcpyHostToDevice) == hipSuccess);
    // slab rows: group_cap per unit, for the rank with the most units; order keys start at -1 (no row)
    const int64_t max_local = (t->total_blocks + s->world - 1) / s->world;
    const int64_t M = (s->n_units > max_local ? s->n_units : max_local) * s->group_cap;
    hs_slab_desc& d = s->desc;
    s->slab_bytes = slab_layout(d, M > 0 ? M : s->group_cap, key_kind, s->key_bytes, P.spec);
    std::vector<uint8_t> slab_image((size_t)s->slab_bytes, 0);
    for (int64_t r = 0; r < d.slab_rows; ++r) ((int64_t*)(slab_image.data() + d.order_off))[r] = -1;
    ok = ok && s->slab.alloc((size_t)s->slab_bytes) &&
         hipMemcpy(s->slab.p, slab_image.data(), slab_image.size(), hipMemcpyHostToDevice) == hipSuccess;
    s->fin = P.fin;
    s->image_bytes = image_layout(s->fin, s->key_bytes, s->merge_cap);
    ok = ok && image_alloc(s->image_host, &s->image_dev, s->image_bytes);
    ok = ok && s->scratch.alloc(hs_agg_finish_scratch_bytes(s->merge_cap, s->fin.n_fold), true);
    if (!ok) {
        hs_set_error("hs_stage: out of device / pinned memory");
        return HS_E_LAUNCH;
    }
    s->n_order = t->total_blocks > 0 ? t->total_blocks : 1;
    s->ready = true;
    return HS_OK;
}

uint32_t* engine_flags(hs_stage* s) { return (uint32_t*)s->engine->flags.p; }

int launch_partial(hs_stage* s, void* stream) {
    const hs_stage_plan& P = s->plan;
    if (s->n_units == 0) return HS_OK;
    if (const int rc = compute_key(s, stream)) return rc;
    return hs_agg_partial_slab(stream, s->cols, P.n_cols, P.key_slot, &P.prog, &P.spec, (const hs_chunk*)s->chunks.p,
                               (const int64_t*)s->chunk0.p, s->n_units, &s->geom, (const int64_t*)s->unit_ids.p,
                               (uint8_t*)s->slab.p, &s->desc, s->ws.p, engine_flags(s), nullptr, nullptr);
}

int launch_finish(hs_stage* s, void* stream, const void* gathered, int32_t world) {
    const hs_stage_plan& P = s->plan;
    return hs_agg_finish(stream, (const uint8_t*)(gathered ? gathered : s->slab.p), world, &s->desc, &s->fin,
                         P.fin_prog.n_ins ? &P.fin_prog : nullptr, s->n_order, s->merge_cap, (uint8_t*)s->image_dev,
                         s->scratch.p, engine_flags(s), (uint32_t*)s->slab.p);
}

}  // namespace

namespace {

// ---- the shared-dictionary tier behind hs_stage_run ------------------------------------------------------------------------
int shared_prepare(hs_stage* s) {
    const hs_stage_plan& P = s->plan;
    s->ready = false;
    if (s->world != 1) {
        hs_set_error("hs_stage: more than 16 groups per block on several ranks belongs to the per-operator ABI");
        return HS_E_LIMIT;
    }
    if (const int rc0 = bind_columns(s)) return rc0;
    const hs_col& kc = s->cols[P.key_slot];
    int32_t key_kind = 0;
    if (const int rck = group_key_shape("hs_stage", kc, key_kind, s->key_bytes)) return rck;
    int rc = hs_agg_shared_geom(s->unit_rows.data(), s->n_units, P.spec.n_acc, s->group_cap, &s->geom);
    if (rc) return rc;
    rc = chunks_upload("hs_stage", s->unit_rows.data(), s->n_units, s->geom, s->chunks);
    if (rc) return rc;
    const int unit_cap = s->geom.pad, n_acc = P.spec.n_acc, nf = s->plan.fin.n_fold;
    s->sh_slots = s->n_units * (int64_t)unit_cap;
    const int64_t slots = s->sh_slots > 0 ? s->sh_slots : 1;
    // result image: the layout of the on-chip path (hs_result_columns / hs_result_write_blockfile read it)
    s->fin = P.fin;
    s->image_bytes = image_layout(s->fin, s->key_bytes, s->merge_cap);
    s->image_dev = nullptr;
    if (!s->ws.alloc(s->geom.ws_bytes, true) || !shared_alloc(s->sh, slots, s->n_units, n_acc, nf, s->merge_cap) ||
        !image_alloc(s->image_host, nullptr, s->image_bytes) || !s->sh.image.alloc((size_t)s->image_bytes, true)) {
        hs_set_error("hs_stage: out of device / pinned memory");
        return HS_E_LAUNCH;
    }
    memset(&s->desc, 0, sizeof(s->desc));
    s->desc.key_kind = key_kind;
    s->desc.key_len = key_kind == HS_STR ? s->key_bytes : 0;
    s->ready = true;
    return HS_OK;
}

// scan with one LDS dictionary per workgroup -> dense partial rows -> merge in unit order -> result columns in the image
int shared_run(hs_stage* s, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const hs_stage_plan& P = s->plan;
    uint32_t* flags = (uint32_t*)s->engine->flags.p;
    const int64_t slots = s->sh_slots;
    s->last_rows = 0;
    if (hipMemsetAsync(flags, 0, 4, stream) != hipSuccess) return HS_E_LAUNCH;
    if (s->n_units == 0 || slots == 0) {
        s->last_flags = 0;
        return HS_OK;
    }
    int rc = compute_key(s, stream);
    if (rc) return rc;
    rc = hs_agg_shared(stream, s->cols, P.n_cols, P.key_slot, &P.prog, &P.spec, (const hs_chunk*)s->chunks.p, s->n_units, &s->geom,
                           (int64_t*)s->sh.rep.p, (uint64_t*)s->sh.acc.p, (int32_t*)s->sh.ngroups.p, s->ws.p, flags, nullptr, nullptr);
    if (rc) return rc;
    return shared_tail(stream, s->sh, P.spec, s->fin, P.fin_prog, s->cols[P.key_slot], s->key_bytes, s->table->nrows, s->n_units,
                       s->geom.pad, slots, s->merge_cap, s->image_host, s->image_bytes, flags, &s->last_flags, &s->last_rows);
}

}  // namespace

namespace {

// past the on-chip tiers with the switch on: the stage moves to the HBM tier and stays there
void hbm_enter(hs_stage* s) {
    if (s->capture) {
        hs_capture_free(s->capture);
        s->capture = nullptr;
    }
    onchip_release(s->image_host, s->image_host_cap, s->sh, s->ws);
    s->image_dev = nullptr;
    s->slab.release();
    s->scratch.release();
    s->tier = 2;
    s->ready = false;
    ++s->tier_switches;
}

int hbm_run(hs_stage* s, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    hs_table* t = s->table;
    const hs_stage_plan& P = s->plan;
    uint32_t* flags = (uint32_t*)s->engine->flags.p;
    s->last_rows = 0;
    s->last_flags = 0;
    if (!s->ready) {
        if (const int rc0 = bind_columns(s)) return rc0;
        int32_t key_kind = 0;
        if (const int rck = group_key_shape("hs_stage", s->cols[P.key_slot], key_kind, s->key_bytes)) return rck;
        memset(&s->desc, 0, sizeof(s->desc));
        s->desc.key_kind = key_kind;
        s->desc.key_len = key_kind == HS_STR ? s->key_bytes : 0;
        s->ready = true;
    }
    s->fin = P.fin;
    if (hipMemsetAsync(flags, 0, 4, stream) != hipSuccess) return HS_E_LAUNCH;
    int rc = compute_key(s, stream);
    if (rc) return rc;
    return hbm_tail(stream, s->hbm, "hs_stage_run", s->cols, P.n_cols, P.key_slot, P.prog, P.spec, s->unit_rows, t->nrows, s->fin,
                    P.fin_prog, s->key_bytes, s->image_host, s->image_host_cap, flags, &s->last_flags, &s->last_rows);
}

}  // namespace

extern "C" int hs_stage_prepare(hs_engine* e, hs_table* t, const hs_stage_plan* plan, size_t plan_bytes, int32_t world,
                                hs_stage** out) {
    if (!e || !t || !plan || !out || plan_bytes != sizeof(hs_stage_plan) || plan->version != HS_STAGE_PLAN_VERSION ||
        plan->n_cols < 1 || plan->n_cols > HS_MAX_COLS || plan->key_slot < 0 || plan->key_slot >= plan->n_cols || world < 1) {
        hs_set_error("hs_stage_prepare: bad plan blob (size %zu, expected %zu)", plan_bytes, sizeof(hs_stage_plan));
        return HS_E_ARG;
    }
    if (hipSetDevice(e->device) != hipSuccess) return HS_E_LAUNCH;
    if (plan->key_computed && (plan->n_kcols < 1 || plan->n_kcols > HS_MAX_COLS || plan->key_prog.n_ins < 1)) {
        hs_set_error("hs_stage_prepare: a computed key needs its program and columns");
        return HS_E_ARG;
    }
    // only the columns the programs name are read from the file
    int32_t want[2 * HS_MAX_COLS];
    int32_t n_want = 0;
    auto add = [&](int32_t c) {
        for (int k = 0; k < n_want; ++k)
            if (want[k] == c) return;
        want[n_want++] = c;
    };
    for (int i = 0; i < plan->n_cols; ++i)
        if (i != plan->key_slot || !plan->key_computed) add(plan->col_ids[i]);
    for (int i = 0; plan->key_computed && i < plan->n_kcols; ++i) add(plan->kcol_ids[i]);
    int rc = n_want ? hs_table_load(e, t, want, n_want) : HS_OK;
    if (rc) return rc;
    hs_stage* s = new hs_stage();
    s->engine = e;
    s->table = t;
    s->plan = *plan;
    s->world = world;
    s->group_cap = plan->group_cap > 0 ? plan->group_cap : 4;
    s->merge_cap = plan->merge_cap > 0 ? plan->merge_cap : 16;
    s->n_units = (int64_t)t->block_rows.size();
    s->unit_rows = rows_before(t->block_rows);
    rc = stage_prepare(s);
    if (rc) {
        delete s;
        return rc;
    }
    *out = s;
    return HS_OK;
}

extern "C" void hs_stage_destroy(hs_stage* s) { delete s; }

// One query on one GPU: scan + partial aggregate -> final merge + projection -> result image on the host.  A dictionary
// overflow (HS_FLAG_DICT_FULL) grows the capacities and runs again; capacities beyond the on-chip tiers: HS_E_LIMIT.
extern "C" int hs_stage_run(hs_stage* s, void* stream, uint32_t* flags_out, int64_t* n_rows_out) {
    if (!s) {
        hs_set_error("hs_stage_run: null stage");
        return HS_E_ARG;
    }
    if (s->world != 1) {
        hs_set_error("hs_stage_run: a multi-rank stage runs as hs_stage_launch_partial / collective / hs_stage_launch_finish");
        return HS_E_ARG;
    }
    for (int attempt = 0; attempt < 14; ++attempt) {
        int rc = HS_OK;
        if (s->tier == 2) {
            // any number of groups: the row-forming pass + the radix tier (not captured: output sizes depend on the data)
            rc = hbm_run(s, stream);
            if (rc) return rc;
            ++s->runs;
            s->last_tier = 2;
            if (flags_out) *flags_out = s->last_flags;
            if (n_rows_out) *n_rows_out = s->last_rows;
            return HS_OK;
        }
        if (s->tier == 1) {
            // tens to thousands of groups per block: shared-dictionary scan + the general operator sequence
            if (!s->ready) rc = shared_prepare(s);
            if (!rc) rc = shared_run(s, stream);
            if (rc == HS_E_LIMIT && s->hbm_on) {  // more rows than the on-chip merge takes, or a shape this tier does not hold
                hbm_enter(s);
                continue;
            }
            if (rc) return rc;
            ++s->runs;
            s->last_tier = 1;
            const SharedNext next = shared_next("hs_stage_run", s->last_flags, s->hbm_on, s->group_cap, s->merge_cap);
            if (next == SharedNext::limit) return HS_E_LIMIT;
            if (next == SharedNext::to_hbm) {
                hbm_enter(s);
                continue;
            }
            if (next == SharedNext::grown) {
                s->ready = false;
                ++s->grows;
                continue;
            }
            if (flags_out) *flags_out = s->last_flags;
            if (n_rows_out) *n_rows_out = s->last_rows;
            return HS_OK;
        }
        if (!s->ready) rc = stage_prepare(s);
        if (rc == HS_E_LIMIT && s->world == 1) {  // the per-lane tables do not hold this query: the shared dictionary may
            s->tier = 1;
            ++s->tier_switches;
            if (s->group_cap < 16) s->group_cap = 16;
            if (s->merge_cap < 64) s->merge_cap = 64;
            continue;
        }
        if (rc) return rc;
        rc = run_or_replay(s->capture, s->runs, s->replays, stream, [&]() {
            const int rcp = launch_partial(s, stream);
            return rcp ? rcp : launch_finish(s, stream, nullptr, 1);
        });
        if (rc) return rc;
        rc = wait_result("hs_stage_run", s->image_host, s->merge_cap, stream, &s->last_flags, &s->last_rows);
        if (rc) return rc;
        ++s->runs;
        s->last_tier = 0;
        if (s->last_flags & (HS_FLAG_DICT_FULL | HS_FLAG_MERGE_FULL)) {
            // more groups than a dictionary was sized for: x2 per workgroup (per-lane tables), x4 for the merge - each
            // grows on its own flag; the merge also keeps up with the per-unit capacity (it holds at least as many keys)
            const bool unit_full = s->last_flags & HS_FLAG_DICT_FULL, merge_full = s->last_flags & HS_FLAG_MERGE_FULL;
            if (merge_full && s->merge_cap >= 4096 && s->hbm_on) {
                hbm_enter(s);
                continue;
            }
            if (merge_full && s->merge_cap >= 4096) {
                hs_set_error("hs_stage_run: GROUP BY cardinality exceeds the on-chip tiers of this path");
                return HS_E_LIMIT;
            }
            if (unit_full && s->group_cap >= 16) {
                // past the per-lane tables: the shared-dictionary tier takes over (round 3; round 2 answered HS_E_LIMIT here)
                if (s->capture) {
                    hs_capture_free(s->capture);
                    s->capture = nullptr;
                }
                s->tier = 1;
                ++s->tier_switches;
                s->group_cap = 64;
                if (s->merge_cap < 256) s->merge_cap = 256;
                s->ready = false;
                s->runs = 0;
                ++s->grows;
                continue;
            }
            if (unit_full) s->group_cap *= 2;
            if (merge_full) s->merge_cap *= 4;
            if (s->merge_cap < 4 * s->group_cap) s->merge_cap = 4 * s->group_cap;
            s->ready = false;
            s->runs = 0;
            ++s->grows;
            continue;
        }
        if (flags_out) *flags_out = s->last_flags;
        if (n_rows_out) *n_rows_out = s->last_rows;
        return HS_OK;
    }
    hs_set_error("hs_stage_run: capacities did not settle");
    return HS_E_LIMIT;
}

// Multi-rank form: launch the rank's scan into its slab, let the caller all-gather the slabs (hs_stage_slab: device
// pointer + bytes), then launch the finish over the gathered slabs and wait.
// (a stage that moved to the HBM tier has none of the buffers these entry points launch on: HS_E_ARG)
extern "C" int hs_stage_launch_partial(hs_stage* s, void* stream) {
    if (!s || s->tier == 2) return HS_E_ARG;
    if (!s->ready) {
        const int rc = stage_prepare(s);
        if (rc) return rc;
    }
    return launch_partial(s, stream);
}
extern "C" void* hs_stage_slab(hs_stage* s, int64_t* bytes) {
    if (!s || !s->ready || s->tier == 2) return nullptr;
    if (bytes) *bytes = s->slab_bytes;
    return s->slab.p;
}
extern "C" int hs_stage_launch_finish(hs_stage* s, void* stream, const void* gathered, int32_t world) {
    if (!s || !s->ready || world < 1 || s->tier == 2) return HS_E_ARG;
    return launch_finish(s, stream, gathered, world);
}
extern "C" int hs_stage_wait(hs_stage* s, void* stream, uint32_t* flags_out, int64_t* n_rows_out) {
    if (!s || !s->ready || s->tier == 2) return HS_E_ARG;
    const int rc = wait_result("hs_stage_run", s->image_host, s->merge_cap, stream, &s->last_flags, &s->last_rows);
    if (rc) return rc;
    if (flags_out) *flags_out = s->last_flags;
    if (n_rows_out) *n_rows_out = s->last_rows;
    return HS_OK;
}
// After HS_FLAG_DICT_FULL / HS_FLAG_MERGE_FULL in the multi-rank form (every rank sees the same flags): grow and prepare again.
extern "C" int hs_stage_grow(hs_stage* s) {
    if (!s || s->tier == 2) return HS_E_ARG;
    const bool unit_full = s->last_flags & HS_FLAG_DICT_FULL, merge_full = s->last_flags & HS_FLAG_MERGE_FULL;
    if ((unit_full && s->group_cap >= 16) || (merge_full && s->merge_cap >= 4096)) return HS_E_LIMIT;
    if (unit_full) s->group_cap *= 2;
    if (merge_full || !unit_full) s->merge_cap = s->merge_cap < 4096 ? s->merge_cap * 4 : s->merge_cap;
    if (s->merge_cap < 4 * s->group_cap) s->merge_cap = 4 * s->group_cap;
    s->ready = false;
    ++s->grows;
    return stage_prepare(s);
}

extern "C" int hs_stage_stats(const hs_stage* s, int64_t* stats) {
    if (!s || !stats) return HS_E_ARG;
    stats[0] = s->runs;
    stats[1] = s->replays;
    stats[2] = s->grows;
    stats[3] = s->group_cap;
    stats[4] = s->merge_cap;
    stats[5] = s->geom.n_chunks;
    return HS_OK;
}

extern "C" int hs_stage_set_hbm_tier(hs_stage* s, int32_t on) {
    if (!s || s->world != 1) {
        hs_set_error("hs_stage_set_hbm_tier: null stage, or a stage of several ranks (the HBM tier runs on one GPU)");
        return HS_E_ARG;
    }
    s->hbm_on = on != 0;
    return HS_OK;
}

extern "C" int hs_stage_tier_stats(const hs_stage* s, int64_t* out) {
    if (!s || !out) {
        hs_set_error("hs_stage_tier_stats: bad arguments");
        return HS_E_ARG;
    }
    out[0] = s->last_tier;
    out[1] = s->hbm.partial_rows;
    out[2] = s->hbm.result_rows;
    out[3] = s->tier_switches;
    return HS_OK;
}

// ---- results -----------------------------------------------------------------------------------------------
extern "C" int hs_result_columns(const hs_stage* s, hs_result_col* out, int32_t cap, int32_t* n) {
    if (!s || !s->ready || !out || !n) {
        hs_set_error("hs_result_columns: bad arguments");
        return HS_E_ARG;
    }
    *n = s->fin.n_out;
    for (int o = 0; o < s->fin.n_out && o < cap; ++o) {
        const hs_finish_out& d = s->fin.outs[o];
        out[o].kind = d.src == 0 ? s->desc.key_kind : d.kind;
        out[o].width = d.src == 0 ? s->key_bytes : (d.kind == HS_I64 ? 8 : 4);
        out[o].data = (const uint8_t*)s->image_host + d.offset;
        out[o].n_rows = s->last_rows;
    }
    return HS_OK;
}

// The result as a one-block BlockFile (reference: WriteToLocalFileTask.write tasks.py:400-410, io.py:47-109): what
// `collect_results` reads back.  Column names / types come from the plan blob.
extern "C" int hs_result_write_blockfile(const hs_stage* s, const char* path) {
    if (!s || !s->ready || !path) {
        hs_set_error("hs_result_write_blockfile: bad arguments");
        return HS_E_ARG;
    }
    // the HBM tier holds any number of rows: blocks of ROWS_PER_BLOCK rows (io.py:217-252)
    return write_image_blockfile("hs_result_write_blockfile", path, s->fin, s->plan.out_types, s->plan.out_names, s->image_host,
                                 s->last_rows, s->desc.key_kind, s->key_bytes, nullptr, s->tier == 2 ? kResultBlockRows : 0);
}

// =====================================================================================================================
// Round 3: the JOIN stage behind the same boundary - the reference's JoinJob (jobs.py:45-79, plan.py:99-109: one per
// shuffle partition; tasks.py:201-240 build + probe, tasks.py:284-289 partial aggregate) and the final stage after it,
// end to end without Python: BlockFile reader for BOTH tables, dictionary coding of the one build-side column the
// aggregate reads, key range, byte table (hs_join8_build), probe inside the aggregate scan (hs_agg_shared_join8), raw unit
// tables -> exchange slab (hs_agg_units_to_slab), finish launch, result image, result BlockFile.  Covers the primary-key /
// foreign-key case of DESIGN.md 4.6 (INTEGER keys, dense key range, unique build keys, GROUP BY the build-side column or a
// probe-side column of at most 4 bytes); anything else returns HS_E_LIMIT and belongs to the per-operator ABI.
// =====================================================================================================================
extern "C" int hs_dict_build(void* stream, const hs_col* col, int64_t nrows, int32_t cap, uint64_t* slot_words, int64_t* slot_reps,
                             int32_t* count, uint32_t* flags);
extern "C" int hs_dict_assign(void* stream, const hs_col* col, int64_t nrows, int32_t cap, uint64_t* slot_words, int64_t* slot_reps,
                              const uint8_t* slot_code, uint8_t* out_codes, uint32_t* flags);
extern "C" int hs_minmax_i32(void* stream, const int32_t* values, int64_t n, int32_t* minmax);

struct hs_join_stage {
    hs_engine* engine = nullptr;
    hs_table *build = nullptr, *probe = nullptr;
    hs_join_stage_plan plan{};
    std::vector<std::string> dict;  // the payload column's distinct strings, sorted: code = index
    DevBuf codes;                   // one code byte per build row
    int32_t key_min = 0;
    int64_t slots = 0;
    DevBuf table, build_ws;
    hs_col cols[HS_MAX_COLS + 1]{};
    hs_agg_geom geom{};
    DevBuf chunks, out_rep, xbuf, ws, slab, scratch;
    int32_t group_cap = 4, merge_cap = 16, unit_cap = 0, n_units = 0, key_bytes = 1, key_kind = HS_STR;
    bool key_is_payload = false, ready = false;
    hs_slab_desc desc{};
    hs_finish_spec fin{};
    int64_t image_bytes = 0;
    void *image_host = nullptr, *image_dev = nullptr, *capture = nullptr;
    int64_t runs = 0, replays = 0, grows = 0;
    uint32_t last_flags = 0;
    int64_t last_rows = 0;
    ~hs_join_stage() {
        if (capture) hs_capture_free(capture);
        if (image_host) (void)hipHostFree(image_host);
    }
};

namespace {

// bytes of row `row` of a STRING column (device) -> host; false on a copy error
bool fetch_string(const hs_col& c, int64_t row, std::string& out) {
    uint8_t len = 0;
    int64_t off = 0;
    if (c.fixed_len >= 0) {
        len = (uint8_t)c.fixed_len;
        off = row * (int64_t)c.fixed_len;
    } else {
        if (hipMemcpy(&len, c.lens + row, 1, hipMemcpyDeviceToHost) != hipSuccess) return false;
        if (hipMemcpy(&off, c.offs + row, 8, hipMemcpyDeviceToHost) != hipSuccess) return false;
    }
    out.assign((size_t)len, '\0');
    return len == 0 || hipMemcpy(&out[0], (const char*)c.data + off, len, hipMemcpyDeviceToHost) == hipSuccess;
}

// Device.dict_encode natively: distinct strings of the column (device set, representative rows read back), sorted, codes
// named BY STRING, one code byte per row.  HS_E_LIMIT when the column has more than 255 distinct values.
// `who`: the stage and column named in the errors; dict / codes: the result
int join_encode_payload(const char* who, const hs_col& col, int64_t n, std::vector<std::string>& dict, DevBuf& codes) {
    const int32_t cap = 4096;
    DevBuf words, reps, state, slot_code;
    if (!words.alloc((size_t)cap * 8) || !reps.alloc((size_t)cap * 8) || !state.alloc(8, true) || !slot_code.alloc(cap, true) ||
        !codes.alloc((size_t)(n > 0 ? n : 1))) {
        hs_set_error("%s: out of device memory", who);
        return HS_E_LAUNCH;
    }
    int rc = hs_dict_build(nullptr, &col, n, cap, (uint64_t*)words.p, (int64_t*)reps.p, (int32_t*)state.p, (uint32_t*)state.p + 1);
    if (rc) return rc;
    int32_t st[2] = {0, 0};
    std::vector<int64_t> host_reps((size_t)cap);
    if (hipMemcpy(st, state.p, 8, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(host_reps.data(), reps.p, (size_t)cap * 8, hipMemcpyDeviceToHost) != hipSuccess)
        return HS_E_LAUNCH;
    if (st[1]) {
        hs_set_error("%s has too many distinct values for a code byte", who);
        return HS_E_LIMIT;
    }
    std::vector<std::pair<int, std::string>> found;  // (slot, string)
    for (int sl = 0; sl < cap; ++sl) {
        if (host_reps[(size_t)sl] < 0) continue;
        std::string text;
        if (!fetch_string(col, host_reps[(size_t)sl], text)) return HS_E_LAUNCH;
        found.emplace_back(sl, std::move(text));
    }
    dict.clear();
    for (const auto& f : found) dict.push_back(f.second);
    std::sort(dict.begin(), dict.end());
    dict.erase(std::unique(dict.begin(), dict.end()), dict.end());
    if (dict.size() > 255) {
        hs_set_error("%s has %zu distinct values (> 255)", who, dict.size());
        return HS_E_LIMIT;
    }
    std::vector<uint8_t> codes_of_slot((size_t)cap, 0);
    for (const auto& f : found)
        codes_of_slot[(size_t)f.first] = (uint8_t)(std::lower_bound(dict.begin(), dict.end(), f.second) - dict.begin());
    if (hipMemcpy(slot_code.p, codes_of_slot.data(), (size_t)cap, hipMemcpyHostToDevice) != hipSuccess) return HS_E_LAUNCH;
    if (n > 0) {
        rc = hs_dict_assign(nullptr, &col, n, cap, (uint64_t*)words.p, (int64_t*)reps.p, (const uint8_t*)slot_code.p, (uint8_t*)codes.p,
                            (uint32_t*)state.p + 1);
        if (rc) return rc;
    }
    if (hipDeviceSynchronize() != hipSuccess) return HS_E_LAUNCH;  // the temporaries above go out of scope
    return HS_OK;
}

int join_prepare_aggregate(hs_join_stage* s) {
    const hs_join_stage_plan& P = s->plan;
    if (s->capture) {
        hs_capture_free(s->capture);
        s->capture = nullptr;
    }
    s->ready = false;
    s->n_units = P.n_parts;
    int cap = 16;
    while (cap < (s->group_cap > 4 ? s->group_cap : 4) * s->n_units) cap *= 2;
    if (cap > 4096) cap = 4096;
    const int64_t unit_rows[2] = {0, s->probe->nrows};
    int rc = hs_agg_shared_units_geom(s->probe->nrows, s->n_units, P.spec.n_acc, cap, 1, &s->geom);
    if (rc) return rc;
    rc = chunks_upload("hs_join_stage", unit_rows, 1, s->geom, s->chunks);
    if (rc) return rc;
    s->unit_cap = s->geom.pad;  // slots of ONE unit's table
    const int64_t slots = (int64_t)s->n_units * s->unit_cap;
    const int n_acc = P.spec.n_acc;
    bool ok = s->out_rep.alloc((size_t)slots * 8) && s->xbuf.alloc((size_t)(16 + slots * 8 * (1 + n_acc)), true) &&
              s->ws.alloc(s->geom.ws_bytes, true);
    // slab: unit u owns rows [u * cap, (u + 1) * cap); zero-filled
    const int64_t slab_bytes = slab_layout(s->desc, slots, s->key_kind, s->key_bytes, P.spec);
    ok = ok && s->slab.alloc((size_t)slab_bytes, true);
    s->fin = P.fin;
    s->image_bytes = image_layout(s->fin, s->key_bytes, s->merge_cap);
    ok = ok && image_alloc(s->image_host, &s->image_dev, s->image_bytes);
    ok = ok && s->scratch.alloc(hs_agg_finish_scratch_bytes(s->merge_cap, s->fin.n_fold), true);
    if (!ok) {
        hs_set_error("hs_join_stage: out of device / pinned memory");
        return HS_E_LAUNCH;
    }
    s->ready = true;
    return HS_OK;
}

int join_launch(hs_join_stage* s, void* stream) {
    const hs_join_stage_plan& P = s->plan;
    uint32_t* flags = (uint32_t*)s->engine->flags.p;
    const hs_col& bk = s->build->cols[P.build_key_col].col;
    int rc = hs_join8_build(stream, (const int32_t*)bk.data, P.build_payload_col >= 0 ? (const uint8_t*)s->codes.p : nullptr,
                            s->build->nrows, 0, nullptr, s->key_min, s->slots, (uint8_t*)s->table.p, s->build_ws.p, flags);
    if (rc) return rc;
    const hs_join8 J{(const uint8_t*)s->table.p, s->slots, s->key_min, P.n_parts};
    const int64_t slots = (int64_t)s->n_units * s->unit_cap;
    uint64_t* keys = (uint64_t*)((char*)s->xbuf.p + 16);
    uint64_t* acc = keys + slots;
    rc = hs_agg_shared_join8(stream, s->cols, P.n_cols + 1, P.key_slot, P.n_cols, &J, s->n_units, &P.prog, &P.spec,
                             (const hs_chunk*)s->chunks.p, &s->geom, (int64_t*)s->out_rep.p, keys, acc, s->ws.p, flags, nullptr, nullptr);
    if (rc) return rc;
    rc = hs_agg_units_to_slab(stream, keys, acc, s->n_units, s->unit_cap, &P.spec, (uint8_t*)s->slab.p, &s->desc, flags);
    if (rc) return rc;
    return hs_agg_finish(stream, (const uint8_t*)s->slab.p, 1, &s->desc, &s->fin, P.fin_prog.n_ins ? &P.fin_prog : nullptr,
                         s->n_units, s->merge_cap, (uint8_t*)s->image_dev, s->scratch.p, flags, (uint32_t*)s->slab.p);
}

}  // namespace

extern "C" int hs_join_stage_prepare(hs_engine* e, hs_table* build, hs_table* probe, const hs_join_stage_plan* plan,
                                     size_t plan_bytes, hs_join_stage** out) {
    if (!e || !build || !probe || !plan || !out || plan_bytes != sizeof(hs_join_stage_plan) ||
        plan->version != HS_JOIN_STAGE_PLAN_VERSION || plan->n_cols < 1 || plan->n_cols >= 8 /* HS_FUSED_COLS: preloaded slots, one is the unit column */ ||
        plan->key_slot < 0 || plan->key_slot >= plan->n_cols || plan->n_parts < 1 || plan->n_parts > 127 ||
        plan->build_key_col < 0 || plan->build_key_col >= (int)build->cols.size() || plan->probe_key_col < 0 ||
        plan->probe_key_col >= (int)probe->cols.size() || plan->build_payload_col >= (int)build->cols.size()) {
        hs_set_error("hs_join_stage_prepare: bad plan blob (size %zu, expected %zu)", plan_bytes, sizeof(hs_join_stage_plan));
        return HS_E_ARG;
    }
    if (hipSetDevice(e->device) != hipSuccess) return HS_E_LAUNCH;
    if (kind_of_type(build->cols[plan->build_key_col].type) != HS_I32 || kind_of_type(probe->cols[plan->probe_key_col].type) != HS_I32) {
        hs_set_error("hs_join_stage_prepare: join keys must be INTEGER columns");
        return HS_E_LIMIT;
    }
    // read what the query references: build key (+ payload), probe key + the program's probe-side columns
    std::vector<int32_t> bcols{plan->build_key_col}, pcols{plan->probe_key_col};
    if (plan->build_payload_col >= 0) bcols.push_back(plan->build_payload_col);
    for (int i = 0; i < plan->n_cols; ++i) {
        if (plan->col_ids[i] >= (int)probe->cols.size()) {
            hs_set_error("hs_join_stage_prepare: slot %d names probe column %d", i, plan->col_ids[i]);
            return HS_E_ARG;
        }
        if (plan->col_ids[i] >= 0) pcols.push_back(plan->col_ids[i]);
    }
    int rc = hs_table_load(e, build, bcols.data(), (int32_t)bcols.size());
    if (!rc) rc = hs_table_load(e, probe, pcols.data(), (int32_t)pcols.size());
    if (rc) return rc;
    if (build->nrows <= 0 || build->nrows >= 0xffffffffll || probe->nrows >= 0xffffffffll) {
        hs_set_error("hs_join_stage_prepare: empty build side or more than 2^32 rows");
        return HS_E_LIMIT;
    }
    hs_join_stage* s = new hs_join_stage();
    s->engine = e;
    s->build = build;
    s->probe = probe;
    s->plan = *plan;
    s->group_cap = plan->group_cap > 0 ? plan->group_cap : 4;
    s->merge_cap = plan->merge_cap > 0 ? plan->merge_cap : 16;
    auto fail = [&](int code) {
        delete s;
        return code;
    };
    if (plan->build_payload_col >= 0) {
        const hs_col& pc = build->cols[plan->build_payload_col].col;
        if (pc.kind != HS_STR) {
            hs_set_error("hs_join_stage_prepare: the build-side column must be a STRING column");
            return fail(HS_E_LIMIT);
        }
        rc = join_encode_payload("hs_join_stage: the build-side column", pc, build->nrows, s->dict, s->codes);
        if (rc) return fail(rc);
    }
    // key range of the build side -> direct addressing
    DevBuf mm;
    int32_t minmax[2] = {0, 0};
    const hs_col& bk = build->cols[plan->build_key_col].col;
    if (!mm.alloc(8) || hs_minmax_i32(nullptr, (const int32_t*)bk.data, build->nrows, (int32_t*)mm.p) != HS_OK ||
        hipMemcpy(minmax, mm.p, 8, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(HS_E_LAUNCH);
    s->key_min = minmax[0];
    s->slots = (int64_t)minmax[1] - (int64_t)minmax[0] + 1;
    if (s->slots > (1ll << 30) || s->slots > 32 * build->nrows) {
        hs_set_error("hs_join_stage_prepare: the build side's key range (%lld slots for %lld keys) is too sparse for the byte table",
                     (long long)s->slots, (long long)build->nrows);
        return fail(HS_E_LIMIT);
    }
    if (!s->table.alloc(hs_join8_table_bytes(s->slots)) || !s->build_ws.alloc(hs_join8_ws_bytes(build->nrows, s->slots))) {
        hs_set_error("hs_join_stage_prepare: out of device memory");
        return fail(HS_E_LAUNCH);
    }
    // column slots of the program: probe-side columns as loaded, the payload as the virtual code column, the unit column last
    const hs_col& pk = probe->cols[plan->probe_key_col].col;
    for (int i = 0; i < plan->n_cols; ++i) {
        if (plan->col_ids[i] >= 0) s->cols[i] = probe->cols[plan->col_ids[i]].col;
        else s->cols[i] = hs_col{HS_JOIN8_CODE, 1, pk.data, nullptr, nullptr};
    }
    s->cols[plan->n_cols] = hs_col{HS_JOIN8_UNIT, -1, pk.data, nullptr, nullptr};
    const hs_col& kc = s->cols[plan->key_slot];
    s->key_is_payload = kc.kind == HS_JOIN8_CODE;
    if (s->key_is_payload) {
        s->key_kind = HS_STR;
        s->key_bytes = 1;
    } else if (kc.kind == HS_I32) {
        s->key_kind = HS_I32;
        s->key_bytes = 4;
    } else if (kc.kind == HS_STR && (kc.fixed_len == 1 || kc.fixed_len == 2 || kc.fixed_len == 4)) {
        s->key_kind = HS_STR;
        s->key_bytes = kc.fixed_len;
    } else {
        hs_set_error("hs_join_stage_prepare: the GROUP BY key must be the build-side column, an INTEGER or a short fixed string");
        return fail(HS_E_LIMIT);
    }
    rc = join_prepare_aggregate(s);
    if (rc) return fail(rc);
    *out = s;
    return HS_OK;
}

extern "C" void hs_join_stage_destroy(hs_join_stage* s) { delete s; }

extern "C" int hs_join_stage_run(hs_join_stage* s, void* stream, uint32_t* flags_out, int64_t* n_rows_out) {
    if (!s) {
        hs_set_error("hs_join_stage_run: null stage");
        return HS_E_ARG;
    }
    for (int attempt = 0; attempt < 12; ++attempt) {
        int rc = HS_OK;
        if (!s->ready) rc = join_prepare_aggregate(s);
        if (rc) return rc;
        rc = run_or_replay(s->capture, s->runs, s->replays, stream, [&]() { return join_launch(s, stream); });
        if (!rc) rc = wait_result("hs_join_stage_run", s->image_host, s->merge_cap, stream, &s->last_flags, &s->last_rows);
        if (rc) return rc;
        ++s->runs;
        if (s->last_flags & HS_FLAG_JOIN_DUP) {
            hs_set_error("hs_join_stage_run: the build side holds a key twice: not a primary-key / foreign-key join (use hs_join_build / count / fill)");
            return HS_E_LIMIT;
        }
        if (s->last_flags & (HS_FLAG_DICT_FULL | HS_FLAG_MERGE_FULL)) {
            const bool unit_full = s->last_flags & HS_FLAG_DICT_FULL, merge_full = s->last_flags & HS_FLAG_MERGE_FULL;
            if ((unit_full && s->group_cap * s->n_units >= 4096) || (merge_full && s->merge_cap >= 4096)) {
                hs_set_error("hs_join_stage_run: GROUP BY cardinality exceeds the on-chip tiers of this path");
                return HS_E_LIMIT;
            }
            if (unit_full) s->group_cap *= 4;
            if (merge_full) s->merge_cap *= 4;
            if (s->merge_cap < 4 * s->group_cap) s->merge_cap = 4 * s->group_cap;
            if (s->merge_cap > 4096) s->merge_cap = 4096;
            s->ready = false;
            s->runs = 0;
            ++s->grows;
            continue;
        }
        if (flags_out) *flags_out = s->last_flags;
        if (n_rows_out) *n_rows_out = s->last_rows;
        return HS_OK;
    }
    hs_set_error("hs_join_stage_run: capacities did not settle");
    return HS_E_LIMIT;
}

extern "C" int hs_join_stage_stats(const hs_join_stage* s, int64_t* stats) {
    if (!s || !stats) return HS_E_ARG;
    stats[0] = s->runs;
    stats[1] = s->replays;
    stats[2] = s->grows;
    stats[3] = s->group_cap;
    stats[4] = s->merge_cap;
    stats[5] = (int64_t)s->dict.size();
    stats[6] = s->slots;
    stats[7] = s->unit_cap;
    return HS_OK;
}

// The result as a one-block BlockFile (tasks.py:400-410, io.py:47-109).  A key that is the build-side column arrives as
// code bytes: decoded through the stage's dictionary here.
extern "C" int hs_join_result_write_blockfile(const hs_join_stage* s, const char* path) {
    if (!s || !s->ready || !path) {
        hs_set_error("hs_join_result_write_blockfile: bad arguments");
        return HS_E_ARG;
    }
    return write_image_blockfile("hs_join_result_write_blockfile", path, s->fin, s->plan.out_types, s->plan.out_names, s->image_host,
                                 s->last_rows, s->key_kind, s->key_bytes, s->key_is_payload ? &s->dict : nullptr);
}

// ---- what the stages that write rows share: the surviving rows of a WHERE, a column gathered through a row list ------------
namespace {

__global__ void __launch_bounds__(256) k_js_iota(int64_t* out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = i;
}

int grid_of(int64_t n) {
    const int64_t g = (n + 255) / 256;
    return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

bool read_i64(hipStream_t stream, const void* dev, int64_t& out) {
    return hipMemcpyAsync(&out, dev, 8, hipMemcpyDeviceToHost, stream) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess;
}

// the rows of one side the WHERE keeps, ascending (every row without a WHERE) -> rows (int64), n_kept
int side_rows(hipStream_t stream, const hs_col* cols, int32_t n_cols, const hs_program& filter, int64_t n, DevBuf& rows,
              int64_t& kept, uint32_t* flags) {
    kept = n;
    if (!rows.alloc((size_t)(n > 0 ? n : 1) * 8)) return HS_E_LAUNCH;
    if (n == 0) return HS_OK;
    if (filter.n_ins == 0) {
        hipLaunchKernelGGL(k_js_iota, dim3(grid_of(n)), dim3(256), 0, stream, (int64_t*)rows.p, n);
        return hipGetLastError() == hipSuccess ? HS_OK : HS_E_LAUNCH;
    }
    DevBuf mask, count, ws;
    if (!mask.alloc((size_t)n) || !count.alloc(8) || !ws.alloc(hs_scan_ws_bytes(n))) return HS_E_LAUNCH;
    void* outs[1] = {mask.p};
    const int32_t kinds[1] = {HS_U8};
    int rc = hs_eval(stream, cols, n_cols, &filter, nullptr, n, nullptr, outs, kinds, 1, flags);
    if (!rc) rc = hs_compact(stream, (const uint8_t*)mask.p, n, (int64_t*)rows.p, (int64_t*)count.p, ws.p);
    if (rc) return rc;
    return read_i64(stream, count.p, kept) ? HS_OK : HS_E_LAUNCH;
}

// column c at rows idx[0 .. n) as a new device column (strings: lens, offsets, payload); out describes it
int gather_col(hipStream_t stream, const hs_col& c, int64_t src_rows, const int64_t* idx, int64_t n, DevBuf& data, DevBuf& lens,
               DevBuf& offs, hs_col& out, int64_t& payload, uint32_t* flags) {
    payload = 0;
    if (c.kind != HS_STR) {
        const int w = elem_bytes(c.kind);
        if (!data.alloc((size_t)(n > 0 ? n : 1) * (size_t)w)) return HS_E_LAUNCH;
        out = hs_col{c.kind, -1, data.p, nullptr, nullptr};
        return n > 0 ? hs_gather_fixed(stream, c.data, w, src_rows, idx, n, nullptr, data.p, flags) : HS_OK;
    }
    DevBuf mm, ws;
    if (!lens.alloc((size_t)(n > 0 ? n : 1)) || !offs.alloc((size_t)(n + 1) * 8, true) || !mm.alloc(8)) return HS_E_LAUNCH;
    if (n > 0) {
        if (!ws.alloc(hs_scan_ws_bytes(n))) return HS_E_LAUNCH;
        int rc = hs_gather_str_lens(stream, &c, src_rows, idx, n, (uint8_t*)lens.p, flags);
        if (!rc) rc = hs_str_offsets(stream, (const uint8_t*)lens.p, n, (int64_t*)offs.p, (int32_t*)mm.p, ws.p);
        if (rc) return rc;
        if (!read_i64(stream, (const int64_t*)offs.p + n, payload)) return HS_E_LAUNCH;
    }
    if (!data.alloc((size_t)(payload > 0 ? payload : 1))) return HS_E_LAUNCH;
    out = hs_col{HS_STR, -1, data.p, (const uint8_t*)lens.p, (const int64_t*)offs.p};
    return n > 0 ? hs_gather_str_bytes(stream, &c, src_rows, idx, n, (const int64_t*)offs.p, (uint8_t*)data.p) : HS_OK;
}

// column c at rows idx[0 .. n) as a result column on the host (the stream is idle afterwards)
int gather_to_host(hipStream_t stream, const hs_col& c, int64_t src_rows, const int64_t* idx, int64_t n, HostCol& out, uint32_t* flags) {
    DevBuf data, lens, offs;
    hs_col g{};
    int64_t payload = 0;
    const int rc = gather_col(stream, c, src_rows, idx, n, data, lens, offs, g, payload, flags);
    if (rc) return rc;
    if (c.kind != HS_STR) {
        out.width = elem_bytes(c.kind);
        out.data.resize((size_t)n * (size_t)out.width);
    } else {
        out.width = -1;
        out.lens.resize((size_t)n);
        out.data.resize((size_t)payload);
        if (hipMemcpyAsync(out.lens.data(), lens.p, (size_t)n, hipMemcpyDeviceToHost, stream) != hipSuccess) return HS_E_LAUNCH;
    }
    if ((!out.data.empty() && hipMemcpyAsync(out.data.data(), data.p, out.data.size(), hipMemcpyDeviceToHost, stream) != hipSuccess) ||
        hipStreamSynchronize(stream) != hipSuccess)
        return HS_E_LAUNCH;
    return HS_OK;
}

// The two tables of a join stage (0 build, 1 probe): every column id in need[side] names a column, the join keys are both
// INTEGER or both STRING, the columns are on the device.  `who` names the entry point in the errors
int join_sides_load(const char* who, hs_engine* e, hs_table* const tables[2], const std::vector<int32_t> need[2], int32_t build_key_col,
                    int32_t probe_key_col) {
    for (int side = 0; side < 2; ++side)
        for (int32_t c : need[side])
            if (c < 0 || c >= (int)tables[side]->cols.size()) {
                hs_set_error("%s: no such column %d in the %s table", who, c, side ? "probe" : "build");
                return HS_E_ARG;
            }
    const int32_t bt = tables[0]->cols[build_key_col].type, pt = tables[1]->cols[probe_key_col].type;
    if (bt != pt || (bt != 0 && bt != 1)) {
        hs_set_error("%s: join keys must be both INTEGER or both STRING (types %d, %d)", who, bt, pt);
        return HS_E_LIMIT;
    }
    if (hipSetDevice(e->device) != hipSuccess) return HS_E_LAUNCH;
    for (int side = 0; side < 2; ++side) {
        const int rc = hs_table_load(e, tables[side], need[side].data(), (int32_t)need[side].size());
        if (rc) return rc;
    }
    return HS_OK;
}

}  // namespace

// =====================================================================================================================
// Round 3: the SELECT / WHERE stage behind the same boundary - a ScanJob whose rows go to the result file
// (jobs.py:45-60; FilterTask tasks.py:167-177, ProjectTask tasks.py:32-35, WriteToLocalFileTask tasks.py:391-410): native
// reader -> predicate (hs_eval) -> stable compaction (hs_compact) -> gathers of the passed-through columns / evaluation of
// the computed ones over the surviving rows (hs_eval with a row list) -> rounding to the stored kinds (hs_quantise) ->
// one device->host copy per column -> BlockFile blocks of ROWS_PER_BLOCK rows, appended in table order.
// =====================================================================================================================
struct hs_select_stage {
    hs_engine* engine = nullptr;
    hs_table* table = nullptr;
    hs_select_stage_plan plan{};
    hs_col cols[HS_MAX_COLS]{}, pcols[HS_MAX_COLS]{};
    std::vector<HostCol> outs;  // last result, host side: per output column the stored values
    int64_t last_rows = 0;
    uint32_t last_flags = 0;
};

extern "C" int hs_select_stage_prepare(hs_engine* e, hs_table* t, const hs_select_stage_plan* plan, size_t plan_bytes,
                                       hs_select_stage** out) {
    if (!e || !t || !plan || !out || plan_bytes != sizeof(hs_select_stage_plan) || plan->version != HS_SELECT_STAGE_PLAN_VERSION ||
        plan->n_cols < 0 || plan->n_cols > HS_MAX_COLS || plan->n_pcols < 0 || plan->n_pcols > HS_MAX_COLS || plan->n_out < 1 ||
        plan->n_out > HS_FINISH_MAX_OUT) {
        hs_set_error("hs_select_stage_prepare: bad plan blob (size %zu, expected %zu)", plan_bytes, sizeof(hs_select_stage_plan));
        return HS_E_ARG;
    }
    if (hipSetDevice(e->device) != hipSuccess) return HS_E_LAUNCH;
    std::vector<int32_t> need(plan->col_ids, plan->col_ids + plan->n_cols);
    need.insert(need.end(), plan->pcol_ids, plan->pcol_ids + plan->n_pcols);
    for (int o = 0; o < plan->n_out; ++o) {
        const int src = plan->out_src[o];
        if (src >= (int)t->cols.size() || (src < 0 && (-1 - src) >= HS_MAX_OUTS)) {
            hs_set_error("hs_select_stage_prepare: output %d is malformed", o);
            return HS_E_ARG;
        }
        if (src >= 0) need.push_back(src);
    }
    for (int32_t c : need) {
        if (c < 0 || c >= (int)t->cols.size()) {
            hs_set_error("hs_select_stage_prepare: no such column %d", c);
            return HS_E_ARG;
        }
    }
    const int rc = hs_table_load(e, t, need.data(), (int32_t)need.size());
    if (rc) return rc;
    hs_select_stage* s = new hs_select_stage();
    s->engine = e;
    s->table = t;
    s->plan = *plan;
    for (int i = 0; i < plan->n_cols; ++i) s->cols[i] = t->cols[plan->col_ids[i]].col;
    for (int i = 0; i < plan->n_pcols; ++i) s->pcols[i] = t->cols[plan->pcol_ids[i]].col;
    *out = s;
    return HS_OK;
}

extern "C" void hs_select_stage_destroy(hs_select_stage* s) { delete s; }

extern "C" int hs_select_stage_run(hs_select_stage* s, void* stream_, uint32_t* flags_out, int64_t* n_rows_out) {
    if (!s) {
        hs_set_error("hs_select_stage_run: null stage");
        return HS_E_ARG;
    }
    hipStream_t stream = (hipStream_t)stream_;
    const hs_select_stage_plan& P = s->plan;
    hs_table* t = s->table;
    const int64_t n = t->nrows;
    uint32_t* flags = (uint32_t*)s->engine->flags.p;
    if (hipMemsetAsync(flags, 0, 4, stream) != hipSuccess) return HS_E_LAUNCH;
    int rc = HS_OK;
    // WHERE: mask -> ascending list of the surviving rows
    DevBuf sel, all_rows;  // all_rows: every row, for the gathers of a STRING column without a WHERE (made once per run)
    int64_t kept = n;
    const bool filtered = P.filter.n_ins > 0;
    if (filtered && n > 0) {
        rc = side_rows(stream, s->cols, P.n_cols, P.filter, n, sel, kept, flags);
        if (rc) return rc;
    }
    const int64_t* rows = filtered && n > 0 ? (const int64_t*)sel.p : nullptr;
    // computed columns over the surviving rows (in-flight f64 / i64), then rounded to what the file stores
    DevBuf computed[HS_MAX_OUTS], stored[HS_MAX_OUTS];
    int n_prog_out = 0;
    for (int o = 0; o < P.n_out; ++o)
        if (P.out_src[o] < 0 && -1 - P.out_src[o] + 1 > n_prog_out) n_prog_out = -1 - P.out_src[o] + 1;
    if (n_prog_out > 0 && kept > 0) {
        void* outs[HS_MAX_OUTS] = {};
        int32_t kinds[HS_MAX_OUTS] = {};
        for (int k = 0; k < n_prog_out; ++k) {
            if (!computed[k].alloc((size_t)kept * 8)) return HS_E_LAUNCH;
            outs[k] = computed[k].p;
            kinds[k] = P.project_kinds[k];
        }
        rc = hs_eval(stream, s->pcols, P.n_pcols, &P.project, rows, kept, nullptr, outs, kinds, n_prog_out, flags);
        for (int k = 0; !rc && k < n_prog_out; ++k) {
            if (!stored[k].alloc((size_t)kept * 4)) return HS_E_LAUNCH;
            rc = hs_quantise(stream, computed[k].p, kinds[k], kept, nullptr, stored[k].p, flags);
        }
        if (rc) return rc;
    }
    // every output column -> host
    s->outs.assign((size_t)P.n_out, HostCol());
    for (int o = 0; o < P.n_out && kept > 0; ++o) {
        HostCol& out = s->outs[(size_t)o];
        const int src = P.out_src[o];
        if (src < 0) {
            out.width = 4;
            out.data.resize((size_t)kept * 4);
            if (hipMemcpyAsync(out.data.data(), stored[-1 - src].p, out.data.size(), hipMemcpyDeviceToHost, stream) != hipSuccess) return HS_E_LAUNCH;
            continue;
        }
        const hs_col& c = t->cols[src].col;
        if (c.kind != HS_STR && !rows) {  // no WHERE: the column as loaded
            out.width = elem_bytes(c.kind);
            out.data.resize((size_t)kept * (size_t)out.width);
            if (hipMemcpyAsync(out.data.data(), c.data, out.data.size(), hipMemcpyDeviceToHost, stream) != hipSuccess) return HS_E_LAUNCH;
            continue;
        }
        const int64_t* idx = rows;
        if (!idx) {  // no WHERE: the gathers of a STRING column still want a row list
            int64_t n_all = 0;
            if (!all_rows.p) rc = side_rows(stream, s->cols, P.n_cols, P.filter, n, all_rows, n_all, flags);
            if (rc) return rc;
            idx = (const int64_t*)all_rows.p;
        }
        rc = gather_to_host(stream, c, n, idx, kept, out, flags);
        if (rc) return rc;
    }
    uint32_t f = 0;
    if (hipMemcpyAsync(&f, flags, 4, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) return HS_E_LAUNCH;
    s->last_flags = f;
    s->last_rows = kept;
    if (flags_out) *flags_out = f;
    if (n_rows_out) *n_rows_out = kept;
    return HS_OK;
}

// The rows of the last run as a BlockFile of rows_per_block-row blocks (reference tasks.py:391-410 + io.py:217-252: a
// result larger than a block continues in further blocks; an empty result writes no file).
extern "C" int hs_select_result_write_blockfile(const hs_select_stage* s, const char* path, int64_t rows_per_block) {
    if (!s || !path || rows_per_block < 1) {
        hs_set_error("hs_select_result_write_blockfile: bad arguments");
        return HS_E_ARG;
    }
    return write_rows_blockfile("hs_select_result_write_blockfile", path, s->plan.n_out, s->plan.out_types, s->plan.out_names, s->outs,
                                s->last_rows, rows_per_block);
}

// =====================================================================================================================
// Round 5: the JOIN-to-rows stage behind the same boundary - a JoinJob whose rows go to the result file (jobs.py:45-79;
// BroadcastHashJoinTask tasks.py:201-240, WriteToLocalFileTask tasks.py:391-410), the engine's _join end to end: native
// reader for both tables -> WHERE per side (hs_eval + hs_compact) -> probe rows in JoinJob order (hs_partition_ids /
// hs_partition_perm) -> join (dense / hashed INTEGER, hashed STRING windows, or the global table) -> pair lists -> gathers
// of every output column through them -> host -> BlockFile blocks of rows_per_block rows.
// =====================================================================================================================
struct hs_join_select_stage {
    hs_engine* engine = nullptr;
    hs_table *build = nullptr, *probe = nullptr;
    hs_join_select_stage_plan plan{};
    hs_col bcols[HS_MAX_COLS]{}, pcols[HS_MAX_COLS]{};
    std::vector<HostCol> outs;
    int64_t runs = 0, last_rows = 0, route = 0, n_build = 0, n_probe = 0;
};

extern "C" int hs_join_select_stage_prepare(hs_engine* e, hs_table* build, hs_table* probe, const hs_join_select_stage_plan* plan,
                                            size_t plan_bytes, hs_join_select_stage** out) {
    if (!e || !build || !probe || !plan || !out || plan_bytes != sizeof(hs_join_select_stage_plan) ||
        plan->version != HS_JOIN_SELECT_STAGE_PLAN_VERSION || plan->n_bcols < 0 || plan->n_bcols > HS_MAX_COLS || plan->n_pcols < 0 ||
        plan->n_pcols > HS_MAX_COLS || plan->n_out < 1 || plan->n_out > HS_FINISH_MAX_OUT || plan->n_parts < 1 || plan->n_parts > 255) {
        hs_set_error("hs_join_select_stage_prepare: bad plan blob (size %zu, expected %zu)", plan_bytes, sizeof(hs_join_select_stage_plan));
        return HS_E_ARG;
    }
    std::vector<int32_t> need[2];
    need[0].assign(plan->bcol_ids, plan->bcol_ids + plan->n_bcols);
    need[1].assign(plan->pcol_ids, plan->pcol_ids + plan->n_pcols);
    need[0].push_back(plan->build_key_col);
    need[1].push_back(plan->probe_key_col);
    for (int o = 0; o < plan->n_out; ++o) {
        if (plan->out_side[o] != 0 && plan->out_side[o] != 1) {
            hs_set_error("hs_join_select_stage_prepare: output %d names no side", o);
            return HS_E_ARG;
        }
        need[plan->out_side[o]].push_back(plan->out_col[o]);
    }
    hs_table* const tables[2] = {build, probe};
    if (const int rc = join_sides_load("hs_join_select_stage_prepare", e, tables, need, plan->build_key_col, plan->probe_key_col)) return rc;
    hs_join_select_stage* s = new hs_join_select_stage();
    s->engine = e;
    s->build = build;
    s->probe = probe;
    s->plan = *plan;
    for (int i = 0; i < plan->n_bcols; ++i) s->bcols[i] = build->cols[plan->bcol_ids[i]].col;
    for (int i = 0; i < plan->n_pcols; ++i) s->pcols[i] = probe->cols[plan->pcol_ids[i]].col;
    *out = s;
    return HS_OK;
}

extern "C" void hs_join_select_stage_destroy(hs_join_select_stage* s) { delete s; }

namespace {

// The join of the compacted key columns (build positions 0 .. nb, probe positions 0 .. np in JoinJob order) -> out_start
// [np + 1], pair lists out_left / out_right (positions), n_out; route: HS_JOIN_ROUTE_*.
struct JoinPairs {
    DevBuf out_start, out_left, out_right;
    int64_t n_out = 0;
    int route = 0;
};

int join_pairs(hipStream_t stream, const hs_col& bk, int64_t nb, const hs_col& pk, int64_t np, uint32_t* flags, JoinPairs& J) {
    DevBuf counts, aux, scan_ws, table, ws, status;
    if (!counts.alloc((size_t)np * 8) || !J.out_start.alloc((size_t)(np + 1) * 8) || !scan_ws.alloc(hs_scan_ws_bytes(np)) ||
        !aux.alloc(hs_join_dense_aux_bytes(np)) || !status.alloc(4, true))
        return HS_E_LAUNCH;
    int32_t lohi[2] = {0, -1};  // the build keys' range, what the dense form is planned from
    if (bk.kind == HS_I32) {
        DevBuf mm;
        if (!mm.alloc(8)) return HS_E_LAUNCH;
        const int rc = hs_minmax_i32(stream, (const int32_t*)bk.data, nb, (int32_t*)mm.p);
        if (rc) return rc;
        if (hipMemcpyAsync(lohi, mm.p, 8, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
            return HS_E_LAUNCH;
    }
    // plan, allocate, build, count - and once more without a route whose window overflowed (hs_join_table_plan owns the rule)
    hs_join_table t{};
    for (uint32_t routes = HS_JOIN_ROUTES_ALL;; routes &= ~HS_JOIN_ROUTE_BIT(t.route)) {
        int rc = hs_join_table_plan(&bk, &pk, nb, np, lohi[0], lohi[1], routes, &t);
        if (rc) return rc;
        if (!t.route) {
            hs_set_error("join_pairs: no join route left for %lld build rows", (long long)nb);
            return HS_E_LIMIT;
        }
        if (!table.alloc((size_t)t.table_bytes) || !ws.alloc((size_t)t.ws_bytes)) return HS_E_LAUNCH;
        rc = hs_join_table_build(stream, &t, &bk, table.p, ws.p, (uint32_t*)status.p, flags);
        if (!rc) rc = hs_join_table_count(stream, &t, &bk, &pk, np, table.p, (int64_t*)counts.p, aux.p);
        if (rc) return rc;
        if (t.route == HS_JOIN_ROUTE_GLOBAL) break;
        uint32_t st = 0;
        if (hipMemcpyAsync(&st, status.p, 4, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
            return HS_E_LAUNCH;
        if (!(st & HS_FLAG_DICT_FULL)) break;
    }
    int rc = hs_exclusive_scan_i64(stream, (const int64_t*)counts.p, np, (int64_t*)J.out_start.p, scan_ws.p);
    if (rc) return rc;
    if (!read_i64(stream, (const int64_t*)J.out_start.p + np, J.n_out)) return HS_E_LAUNCH;
    if (!J.out_left.alloc((size_t)(J.n_out > 0 ? J.n_out : 1) * 8) || !J.out_right.alloc((size_t)(J.n_out > 0 ? J.n_out : 1) * 8))
        return HS_E_LAUNCH;
    if (J.n_out > 0)
        rc = hs_join_table_fill(stream, &t, &bk, &pk, np, table.p, aux.p, (const int64_t*)J.out_start.p, (int64_t*)J.out_left.p,
                                (int64_t*)J.out_right.p);
    J.route = t.route;
    return rc;
}

// The first part of a join stage's run (tasks.py:201-240): the WHERE per side, the probe rows in JoinJob order, the join over
// the key columns of the surviving rows, the table rows of every pair.  pstart: JoinJob starts among the ordered probe rows.
struct JoinedRows {
    DevBuf brows, porder, pstart, bidx, pidx;  // bidx / pidx: build / probe table row of every pair
    JoinPairs J;
    int64_t nb = 0, np = 0;
};

int join_rows(hipStream_t stream, hs_table* build, hs_table* probe, int32_t build_key_col, int32_t probe_key_col, int32_t n_parts,
              const hs_col* bcols, int32_t n_bcols, const hs_program& build_filter, const hs_col* pcols, int32_t n_pcols,
              const hs_program& probe_filter, uint32_t* flags, JoinedRows& R) {
    const int64_t nb_all = build->nrows, np_all = probe->nrows;
    const hs_col& bkey = build->cols[build_key_col].col;
    const hs_col& pkey = probe->cols[probe_key_col].col;
    // 1. WHERE per side
    DevBuf prows;
    int64_t nb = 0, np = 0;
    int rc = side_rows(stream, bcols, n_bcols, build_filter, nb_all, R.brows, nb, flags);
    if (!rc) rc = side_rows(stream, pcols, n_pcols, probe_filter, np_all, prows, np, flags);
    if (rc) return rc;
    R.nb = nb;
    R.np = np;
    // 2. probe rows in JoinJob order: partition ids of the surviving rows, a stable counting sort, the row ids through it
    DevBuf part, perm, pws;
    if (!R.porder.alloc((size_t)(np > 0 ? np : 1) * 8) || !R.pstart.alloc((size_t)(n_parts + 1) * 8, true)) return HS_E_LAUNCH;
    if (np > 0) {
        if (!part.alloc((size_t)np) || !perm.alloc((size_t)np * 8) || !pws.alloc(hs_partition_ws_bytes(np, n_parts)))
            return HS_E_LAUNCH;
        rc = hs_partition_ids(stream, &pkey, (const int64_t*)prows.p, np, n_parts, (uint8_t*)part.p);
        if (!rc) rc = hs_partition_perm(stream, (const uint8_t*)part.p, np, n_parts, (int64_t*)perm.p, (int64_t*)R.pstart.p, pws.p);
        if (!rc) rc = hs_gather_fixed(stream, prows.p, 8, np, (const int64_t*)perm.p, np, nullptr, R.porder.p, flags);
        if (rc) return rc;
    }
    // 3. the join over the key columns of the surviving rows
    if (nb > 0 && np > 0) {
        DevBuf bk_data, bk_lens, bk_offs, pk_data, pk_lens, pk_offs;
        hs_col bk{}, pk{};
        int64_t payload = 0;
        rc = gather_col(stream, bkey, nb_all, (const int64_t*)R.brows.p, nb, bk_data, bk_lens, bk_offs, bk, payload, flags);
        if (!rc) rc = gather_col(stream, pkey, np_all, (const int64_t*)R.porder.p, np, pk_data, pk_lens, pk_offs, pk, payload, flags);
        if (!rc) rc = join_pairs(stream, bk, nb, pk, np, flags, R.J);
        if (rc) return rc;
    }
    // 4. table rows of every pair
    const int64_t n_out = R.J.n_out;
    if (n_out > 0) {
        if (!R.bidx.alloc((size_t)n_out * 8) || !R.pidx.alloc((size_t)n_out * 8)) return HS_E_LAUNCH;
        rc = hs_gather_fixed(stream, R.brows.p, 8, nb, (const int64_t*)R.J.out_left.p, n_out, nullptr, R.bidx.p, flags);
        if (!rc) rc = hs_gather_fixed(stream, R.porder.p, 8, np, (const int64_t*)R.J.out_right.p, n_out, nullptr, R.pidx.p, flags);
        if (rc) return rc;
    }
    return HS_OK;
}

}  // namespace

extern "C" int hs_join_select_stage_run(hs_join_select_stage* s, void* stream_, uint32_t* flags_out, int64_t* n_rows_out) {
    if (!s) {
        hs_set_error("hs_join_select_stage_run: null stage");
        return HS_E_ARG;
    }
    if (hipSetDevice(s->engine->device) != hipSuccess) return HS_E_LAUNCH;
    hipStream_t stream = (hipStream_t)stream_;
    const hs_join_select_stage_plan& P = s->plan;
    uint32_t* flags = (uint32_t*)s->engine->flags.p;
    if (hipMemsetAsync(flags, 0, 4, stream) != hipSuccess) return HS_E_LAUNCH;
    JoinedRows R;
    int rc = join_rows(stream, s->build, s->probe, P.build_key_col, P.probe_key_col, P.n_parts, s->bcols, P.n_bcols, P.build_filter,
                       s->pcols, P.n_pcols, P.probe_filter, flags, R);
    if (rc) return rc;
    // every output column through the pair rows -> host
    const int64_t n_out = R.J.n_out;
    s->outs.assign((size_t)P.n_out, HostCol());
    for (int o = 0; o < P.n_out && n_out > 0; ++o) {
        hs_table* t = P.out_side[o] ? s->probe : s->build;
        const hs_col& c = t->cols[P.out_col[o]].col;
        rc = gather_to_host(stream, c, t->nrows, (const int64_t*)(P.out_side[o] ? R.pidx.p : R.bidx.p), n_out, s->outs[(size_t)o], flags);
        if (rc) return rc;
    }
    uint32_t f = 0;
    if (hipMemcpyAsync(&f, flags, 4, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) return HS_E_LAUNCH;
    s->runs += 1;
    s->last_rows = n_out;
    s->route = R.J.route;
    s->n_build = R.nb;
    s->n_probe = R.np;
    if (flags_out) *flags_out = f;
    if (n_rows_out) *n_rows_out = n_out;
    return HS_OK;
}

extern "C" int hs_join_select_stage_stats(const hs_join_select_stage* s, int64_t* stats) {
    if (!s || !stats) {
        hs_set_error("hs_join_select_stage_stats: bad arguments");
        return HS_E_ARG;
    }
    stats[0] = s->runs;
    stats[1] = s->last_rows;
    stats[2] = s->route;
    stats[3] = s->n_build;
    stats[4] = s->n_probe;
    return HS_OK;
}

// The rows of the last run as a BlockFile of rows_per_block-row blocks (as hs_select_result_write_blockfile)
extern "C" int hs_join_select_result_write_blockfile(const hs_join_select_stage* s, const char* path, int64_t rows_per_block) {
    if (!s || !path || rows_per_block < 1) {
        hs_set_error("hs_join_select_result_write_blockfile: bad arguments");
        return HS_E_ARG;
    }
    return write_rows_blockfile("hs_join_select_result_write_blockfile", path, s->plan.n_out, s->plan.out_types, s->plan.out_names,
                                s->outs, s->last_rows, rows_per_block);
}

// =====================================================================================================================
// Round 5: the general JOIN feeding a GROUP BY behind the same boundary - the reference's JoinJob for every join
// (tasks.py:201-240 build + probe, tasks.py:284-289 partial aggregate, plan.py:99-109) and the final stage after it.  The
// join is hs_join_select_stage_run's (join_rows); the pairs of one JoinJob are one row-range unit of the shared-dictionary
// scan, which reads every slot's column gathered through the pair rows; the tail is the scan stage's (shared_tail).
// =====================================================================================================================
struct hs_join_group_stage {
    hs_engine* engine = nullptr;
    hs_table *build = nullptr, *probe = nullptr;
    hs_join_group_stage_plan plan{};
    hs_col bcols[HS_MAX_COLS]{}, pcols[HS_MAX_COLS]{};  // the side filters' columns
    hs_col src[HS_MAX_COLS]{};                          // table column behind every slot (a coded key: its code bytes)
    std::vector<std::string> dict;                      // a coded GROUP BY key's strings, sorted: code = index
    DevBuf codes;                                       // one code byte per row of the key's table
    bool key_coded = false;
    int32_t key_kind = HS_I32, key_bytes = 4;
    // the last run's pairs and the slots' columns through them (a capacity retry aggregates them again): numeric argument
    // slots as HS_PAIR columns (table column + pair rows, read by the compiled scan), the others gathered
    JoinedRows R;
    int32_t agg_route = HS_JOIN_AGG_PAIRS;
    DevBuf gdata[HS_MAX_COLS], glens[HS_MAX_COLS], goffs[HS_MAX_COLS];
    hs_col cols[HS_MAX_COLS]{};
    std::vector<int64_t> unit_rows;  // pairs before JoinJob u, u = 0 .. n_parts
    // the aggregate over the pairs (rebuilt when a capacity grows)
    bool ready = false;
    int32_t group_cap = 16, merge_cap = 64;
    hs_agg_geom geom{};
    DevBuf chunks, ws;
    SharedBufs sh;
    hs_finish_spec fin{};
    int64_t slots = 0, image_bytes = 0;
    void* image_host = nullptr;
    int64_t runs = 0, grows = 0;
    // the HBM (radix) tier, taken past the on-chip tiers when the stage's switch is on (sticky)
    bool hbm_on = false, hbm = false;
    HbmBufs hbm_bufs;
    size_t image_host_cap = 0;
    int32_t last_tier = 1;
    int64_t tier_switches = 0;
    uint32_t last_flags = 0;
    int64_t last_rows = 0;
    ~hs_join_group_stage() {
        if (image_host) (void)hipHostFree(image_host);
    }
};

extern "C" int hs_join_group_stage_prepare(hs_engine* e, hs_table* build, hs_table* probe, const hs_join_group_stage_plan* plan,
                                           size_t plan_bytes, hs_join_group_stage** out) {
    if (!e || !build || !probe || !plan || !out || plan_bytes != sizeof(hs_join_group_stage_plan) ||
        plan->version != HS_JOIN_GROUP_STAGE_PLAN_VERSION || plan->n_bcols < 0 || plan->n_bcols > HS_MAX_COLS || plan->n_pcols < 0 ||
        plan->n_pcols > HS_MAX_COLS || plan->n_cols < 1 || plan->n_cols > HS_FUSED_COLS || plan->key_slot < 0 ||
        plan->key_slot >= plan->n_cols || plan->n_parts < 1 || plan->n_parts > 255 || plan->fin.n_out < 1 ||
        plan->fin.n_out > HS_FINISH_MAX_OUT) {
        hs_set_error("hs_join_group_stage_prepare: bad plan blob (size %zu, expected %zu)", plan_bytes, sizeof(hs_join_group_stage_plan));
        return HS_E_ARG;
    }
    std::vector<int32_t> need[2];
    need[0].assign(plan->bcol_ids, plan->bcol_ids + plan->n_bcols);
    need[1].assign(plan->pcol_ids, plan->pcol_ids + plan->n_pcols);
    need[0].push_back(plan->build_key_col);
    need[1].push_back(plan->probe_key_col);
    for (int i = 0; i < plan->n_cols; ++i) {
        if (plan->col_side[i] != 0 && plan->col_side[i] != 1) {
            hs_set_error("hs_join_group_stage_prepare: slot %d names no side", i);
            return HS_E_ARG;
        }
        need[plan->col_side[i]].push_back(plan->col_ids[i]);
    }
    hs_table* const tables[2] = {build, probe};
    if (const int rc = join_sides_load("hs_join_group_stage_prepare", e, tables, need, plan->build_key_col, plan->probe_key_col)) return rc;
    hs_join_group_stage* s = new hs_join_group_stage();
    s->engine = e;
    s->build = build;
    s->probe = probe;
    s->plan = *plan;
    // starting capacities: powers of two (the geometry and the x4 growth need them), at most the on-chip tiers' 4096
    while (s->group_cap < plan->group_cap && s->group_cap < 4096) s->group_cap *= 2;
    while (s->merge_cap < plan->merge_cap && s->merge_cap < 4096) s->merge_cap *= 2;
    for (int i = 0; i < plan->n_bcols; ++i) s->bcols[i] = build->cols[plan->bcol_ids[i]].col;
    for (int i = 0; i < plan->n_pcols; ++i) s->pcols[i] = probe->cols[plan->pcol_ids[i]].col;
    for (int i = 0; i < plan->n_cols; ++i) s->src[i] = tables[plan->col_side[i]]->cols[plan->col_ids[i]].col;
    // the GROUP BY key: INTEGER / FLOAT / TIMESTAMP and 1 / 2 / 4-byte strings as stored, other strings as code bytes
    const hs_table* kt = tables[plan->col_side[plan->key_slot]];
    hs_col& kc = s->src[plan->key_slot];
    if (kc.kind == HS_STR && kc.fixed_len != 1 && kc.fixed_len != 2 && kc.fixed_len != 4) {
        const int rc = kt->nrows > 0 ? join_encode_payload("hs_join_group_stage: the GROUP BY column", kc, kt->nrows, s->dict, s->codes)
                                     : (s->codes.alloc(1, true) ? HS_OK : HS_E_LAUNCH);
        if (rc) {
            delete s;
            return rc;
        }
        kc = hs_col{HS_STR, 1, s->codes.p, nullptr, nullptr};
        s->key_coded = true;
    }
    if (const int rc = group_key_shape("hs_join_group_stage_prepare", kc, s->key_kind, s->key_bytes)) {
        delete s;
        return rc;
    }
    *out = s;
    return HS_OK;
}

extern "C" void hs_join_group_stage_destroy(hs_join_group_stage* s) { delete s; }

namespace {

// geometry, unit tables and result image of the aggregate over the pairs, at the stage's current capacities
int join_group_prepare(hs_join_group_stage* s) {
    const hs_join_group_stage_plan& P = s->plan;
    s->ready = false;
    const int64_t n_units = P.n_parts;
    int rc = hs_agg_shared_geom(s->unit_rows.data(), n_units, P.spec.n_acc, s->group_cap, &s->geom);
    if (rc) return rc;
    rc = chunks_upload("hs_join_group_stage", s->unit_rows.data(), n_units, s->geom, s->chunks);
    if (rc) return rc;
    s->slots = n_units * (int64_t)s->geom.pad;
    s->fin = P.fin;
    s->image_bytes = image_layout(s->fin, s->key_bytes, s->merge_cap);
    if (!s->ws.alloc(s->geom.ws_bytes, true) || !shared_alloc(s->sh, s->slots, n_units, P.spec.n_acc, P.fin.n_fold, s->merge_cap) ||
        !image_alloc(s->image_host, nullptr, s->image_bytes) || !s->sh.image.alloc((size_t)s->image_bytes, true)) {
        hs_set_error("hs_join_group_stage: out of device / pinned memory");
        return HS_E_LAUNCH;
    }
    s->ready = true;
    return HS_OK;
}

// every slot's column over the pairs: with `pairs`, a numeric argument slot is the table column read through the pair rows
// (HS_PAIR); the key and the string slots - and every slot without `pairs` - are gathered through them
int join_group_columns(hs_join_group_stage* s, hipStream_t stream, uint32_t* flags, bool pairs) {
    const hs_join_group_stage_plan& P = s->plan;
    const int64_t n = s->R.J.n_out;
    s->agg_route = pairs ? HS_JOIN_AGG_PAIRS : HS_JOIN_AGG_GATHERED;
    for (int i = 0; i < P.n_cols; ++i) {
        const hs_table* t = P.col_side[i] ? s->probe : s->build;
        const int64_t* idx = (const int64_t*)(P.col_side[i] ? s->R.pidx.p : s->R.bidx.p);
        const hs_col& c = s->src[i];
        int rc = HS_OK;
        if (pairs && i != P.key_slot && (c.kind == HS_I32 || c.kind == HS_F32 || c.kind == HS_I64)) {
            s->gdata[i].release();
            s->cols[i] = hs_col{HS_PAIR | c.kind, -1, c.data, nullptr, idx};
        } else if (c.kind == HS_STR && i == P.key_slot) {  // a fixed-width key stays fixed-width: the scan packs it into the key word
            if (!s->gdata[i].alloc((size_t)n * (size_t)c.fixed_len)) return HS_E_LAUNCH;
            rc = hs_gather_fixed(stream, c.data, c.fixed_len, t->nrows, idx, n, nullptr, s->gdata[i].p, flags);
            s->cols[i] = hs_col{HS_STR, c.fixed_len, s->gdata[i].p, nullptr, nullptr};
        } else {
            int64_t payload = 0;
            rc = gather_col(stream, c, t->nrows, idx, n, s->gdata[i], s->glens[i], s->goffs[i], s->cols[i], payload, flags);
        }
        if (rc) return rc;
    }
    return HS_OK;
}

// the join, the JoinJob boundaries among the pairs, every slot's column over the pairs
int join_group_pairs(hs_join_group_stage* s, hipStream_t stream, uint32_t* flags) {
    const hs_join_group_stage_plan& P = s->plan;
    s->R = JoinedRows();  // the previous run's pairs go before this run's are made (peak HBM: one set)
    for (int i = 0; i < HS_MAX_COLS; ++i) {
        s->gdata[i].release();
        s->glens[i].release();
        s->goffs[i].release();
    }
    JoinedRows R;
    int rc = join_rows(stream, s->build, s->probe, P.build_key_col, P.probe_key_col, P.n_parts, s->bcols, P.n_bcols, P.build_filter,
                       s->pcols, P.n_pcols, P.probe_filter, flags, R);
    if (rc) return rc;
    R.J.out_left.release();  // (the table rows of the pairs are in bidx / pidx)
    R.J.out_right.release();
    s->R = std::move(R);
    const int64_t n = s->R.J.n_out;
    std::vector<int64_t> unit_rows((size_t)P.n_parts + 1, 0);
    if (n > 0) {
        // the compiled scan reads a lane's four pair rows at once: the 4 past the last pair hold row 0, not stale bytes
        if (hipMemsetAsync((char*)s->R.bidx.p + n * 8, 0, 32, stream) != hipSuccess ||
            hipMemsetAsync((char*)s->R.pidx.p + n * 8, 0, 32, stream) != hipSuccess)
            return HS_E_LAUNCH;
        // JoinJob u's pairs start where its first probe row's do: out_start at the partition starts, one readback
        DevBuf starts;
        if (!starts.alloc((size_t)(P.n_parts + 1) * 8)) return HS_E_LAUNCH;
        rc = hs_gather_fixed(stream, s->R.J.out_start.p, 8, s->R.np + 1, (const int64_t*)s->R.pstart.p, P.n_parts + 1, nullptr, starts.p, flags);
        if (rc) return rc;
        if (hipMemcpyAsync(unit_rows.data(), starts.p, (size_t)(P.n_parts + 1) * 8, hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess)
            return HS_E_LAUNCH;
        unit_rows[0] = 0;
        unit_rows[(size_t)P.n_parts] = n;
    }
    if (unit_rows != s->unit_rows) s->ready = false;  // the chunk geometry follows the JoinJob boundaries
    s->unit_rows = std::move(unit_rows);
    if (n == 0) return HS_OK;
    return join_group_columns(s, stream, flags, hs_jit_get_enabled() != 0 && !s->hbm);  // (the HBM tier reads gathered columns)
}

}  // namespace

// One query on one GPU: join -> aggregate over the pairs -> final merge + projection -> result image on the host.  A
// dictionary overflow grows the capacities and aggregates the same pairs again; beyond the on-chip tiers: HS_E_LIMIT.
extern "C" int hs_join_group_stage_run(hs_join_group_stage* s, void* stream_, uint32_t* flags_out, int64_t* n_rows_out) {
    if (!s) {
        hs_set_error("hs_join_group_stage_run: null stage");
        return HS_E_ARG;
    }
    if (hipSetDevice(s->engine->device) != hipSuccess) return HS_E_LAUNCH;
    hipStream_t stream = (hipStream_t)stream_;
    const hs_join_group_stage_plan& P = s->plan;
    uint32_t* flags = (uint32_t*)s->engine->flags.p;
    if (hipMemsetAsync(flags, 0, 4, stream) != hipSuccess) return HS_E_LAUNCH;
    int rc = join_group_pairs(s, stream, flags);
    if (rc) return rc;
    uint32_t join_flags = 0;  // errors of the side filters and gathers (the aggregate starts from clear flags)
    if (hipMemcpyAsync(&join_flags, flags, 4, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
        return HS_E_LAUNCH;
    ++s->runs;
    s->last_rows = 0;
    s->last_flags = join_flags;
    const int64_t n_pairs = s->R.J.n_out;
    // past the on-chip tiers with the switch on: the stage moves to the HBM tier and stays there
    auto hbm_enter = [&]() {
        onchip_release(s->image_host, s->image_host_cap, s->sh, s->ws);
        s->chunks.release();
        s->ready = false;
        s->hbm = true;
        ++s->tier_switches;
    };
    for (int attempt = 0; n_pairs > 0 && attempt < 14; ++attempt) {
        s->last_rows = 0;
        if (s->hbm) {
            // any number of groups: the JoinJobs' pair ranges are the units of the row-forming pass + the radix tier
            if (s->agg_route != HS_JOIN_AGG_GATHERED) rc = join_group_columns(s, stream, flags, false);
            if (rc) return rc;
            if (hipMemsetAsync(flags, 0, 4, stream) != hipSuccess) return HS_E_LAUNCH;
            s->fin = P.fin;
            uint32_t f = 0;
            rc = hbm_tail(stream, s->hbm_bufs, "hs_join_group_stage_run", s->cols, P.n_cols, P.key_slot, P.prog, P.spec, s->unit_rows, n_pairs,
                          s->fin, P.fin_prog, s->key_bytes, s->image_host, s->image_host_cap, flags, &f, &s->last_rows);
            if (rc) return rc;
            s->last_tier = 2;
            s->last_flags = join_flags | f;
            if (flags_out) *flags_out = s->last_flags;
            if (n_rows_out) *n_rows_out = s->last_rows;
            return HS_OK;
        }
        if (!s->ready) rc = join_group_prepare(s);
        if (rc == HS_E_LIMIT && s->hbm_on) {
            hbm_enter();
            rc = HS_OK;
            continue;
        }
        if (rc) return rc;
        if (hipMemsetAsync(flags, 0, 4, stream) != hipSuccess) return HS_E_LAUNCH;
        rc = hs_agg_shared(stream, s->cols, P.n_cols, P.key_slot, &P.prog, &P.spec, (const hs_chunk*)s->chunks.p, P.n_parts, &s->geom,
                           (int64_t*)s->sh.rep.p, (uint64_t*)s->sh.acc.p, (int32_t*)s->sh.ngroups.p, s->ws.p, flags, nullptr, nullptr);
        if (rc == HS_E_LIMIT && s->agg_route == HS_JOIN_AGG_PAIRS) {
            // the run-time compiler could not take this program: the interpreter reads the same columns gathered
            rc = join_group_columns(s, stream, flags, false);
            if (rc) return rc;
            continue;
        }
        uint32_t f = 0;
        if (!rc)
            rc = shared_tail(stream, s->sh, P.spec, s->fin, P.fin_prog, s->cols[P.key_slot], s->key_bytes, n_pairs, P.n_parts, s->geom.pad,
                             s->slots, s->merge_cap, s->image_host, s->image_bytes, flags, &f, &s->last_rows);
        if (rc == HS_E_LIMIT && s->hbm_on) {  // more rows than the on-chip merge takes, or a shape this tier does not hold
            hbm_enter();
            rc = HS_OK;
            continue;
        }
        if (rc) return rc;
        s->last_tier = 1;
        const SharedNext next = shared_next("hs_join_group_stage_run", f, s->hbm_on, s->group_cap, s->merge_cap);
        if (next == SharedNext::limit) return HS_E_LIMIT;
        if (next == SharedNext::to_hbm) {
            hbm_enter();
            continue;
        }
        if (next == SharedNext::grown) {
            s->ready = false;
            ++s->grows;
            continue;
        }
        s->last_flags = join_flags | f;
        if (flags_out) *flags_out = s->last_flags;
        if (n_rows_out) *n_rows_out = s->last_rows;
        return HS_OK;
    }
    if (n_pairs > 0) {
        hs_set_error("hs_join_group_stage_run: capacities did not settle");
        return HS_E_LIMIT;
    }
    if (flags_out) *flags_out = s->last_flags;
    if (n_rows_out) *n_rows_out = 0;
    return HS_OK;
}

extern "C" int hs_join_group_stage_set_hbm_tier(hs_join_group_stage* s, int32_t on) {
    if (!s) {
        hs_set_error("hs_join_group_stage_set_hbm_tier: null stage");
        return HS_E_ARG;
    }
    s->hbm_on = on != 0;
    return HS_OK;
}

extern "C" int hs_join_group_stage_tier_stats(const hs_join_group_stage* s, int64_t* out) {
    if (!s || !out) {
        hs_set_error("hs_join_group_stage_tier_stats: bad arguments");
        return HS_E_ARG;
    }
    out[0] = s->last_tier;
    out[1] = s->hbm_bufs.partial_rows;
    out[2] = s->hbm_bufs.result_rows;
    out[3] = s->tier_switches;
    return HS_OK;
}

extern "C" int hs_join_group_stage_stats(const hs_join_group_stage* s, int64_t* stats) {
    if (!s || !stats) {
        hs_set_error("hs_join_group_stage_stats: bad arguments");
        return HS_E_ARG;
    }
    stats[0] = s->runs;
    stats[1] = s->grows;
    stats[2] = s->group_cap;
    stats[3] = s->merge_cap;
    stats[4] = s->R.J.route;
    stats[5] = s->agg_route;
    stats[6] = s->R.J.n_out;
    stats[7] = s->R.nb;
    stats[8] = s->R.np;
    stats[9] = (int64_t)s->dict.size();
    return HS_OK;
}

// The result as a one-block BlockFile; a coded key is decoded through the stage's dictionary (as hs_join_result_write_blockfile)
extern "C" int hs_join_group_result_write_blockfile(const hs_join_group_stage* s, const char* path) {
    if (!s || !path || (s->last_rows > 0 && ((!s->ready && !s->hbm) || !s->image_host))) {
        hs_set_error("hs_join_group_result_write_blockfile: bad arguments");
        return HS_E_ARG;
    }
    return write_image_blockfile("hs_join_group_result_write_blockfile", path, s->fin, s->plan.out_types, s->plan.out_names,
                                 s->image_host, s->last_rows, s->key_kind, s->key_bytes, s->key_coded ? &s->dict : nullptr,
                                 s->hbm ? kResultBlockRows : 0);
}
