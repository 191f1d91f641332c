// CDNA4 (gfx950 / MI355X) GPU library for the covalent SSH executor.
//
// New MI355X-native component with no reference counterpart (the
// reference plugin, /root/reference/covalent_ssh_plugin, has zero native
// code — SURVEY.md §2.4).  Provides, behind a plain C ABI consumed via
// ctypes (so the remote stub needs no torch and no Python extension ABI):
//
//   * csp_probe_json  — device probe + measured HBM bandwidth and bf16
//                       MFMA throughput from the two hand-written
//                       warm-up kernels below,
//   * csp_warmup      — clock/cache warm-up (MFMA spin + HBM sweep)
//                       bounded by a millisecond budget,
//   * csp_host_alloc / csp_host_free / csp_staging_get /
//     csp_memcpy_d2h / csp_memcpy_h2d
//                     — hipHostMalloc-pinned staging for large tensor
//                       results on the SFTP/stdout return path,
//   * csp_d2h_stream_fd
//                     — a large tensor result framed straight onto the
//                       worker's channel fd, its D2H copy overlapped with
//                       the pipe writes through a two-chunk pinned ring,
//   * csp_h2d_stream_fd
//                     — the mirror for large tensor arguments: a frame read
//                       from the channel fd lands in HBM chunk by chunk, the
//                       H2D copy overlapped with the reads,
//   * csp_checksum_dev — two-word integer checksum of a device buffer (the
//                       worker compares it with the dispatcher's),
//   * csp_copy_checksum_dev
//                     — device-to-device copy that yields the same checksum
//                       in the same pass (a cached argument's private copy),
//   * csp_pack_dev    — one launch gathers many small device buffers into a
//                       contiguous zero-padded arena, so a result of hundreds
//                       of small tensors leaves as one streamed frame,
//   * csp_pack_checksum_dev
//                     — the same gather with the arena's checksum from the
//                       same pass; with one segment, a checksummed copy from a
//                       source of any alignment (a result kept in HBM as a
//                       master for reuse as an argument),
//   * csp_unpack_checksum_dev
//                     — the mirror for arguments: one launch scatters an
//                       arena of many small tensor arguments into private
//                       per-tensor buffers and yields the arena's checksum in
//                       the same pass,
//   * csp_patch_unpack_checksum_dev
//                     — the same pass over a cached arena of which a few
//                       segments changed: the changed segments, sent as a
//                       small delta arena, are written over the held master
//                       in place while the whole new arena is scattered and
//                       checksummed,
//   * csp_rebase_unpack_checksum_dev
//                     — the same pass for a NEW arena of any layout: every
//                       segment comes from a held arena, wherever it lies
//                       there, or from a small delta arena, and the new arena
//                       is written out as a new master while it is scattered
//                       and checksummed; the held arena is only read,
//   * csp_hbm_sweep_dev
//                     — one launch of the probe's HBM sweep kernel on the
//                       caller's buffers (tests: what the sweep copies),
//   * csp_checksum_grid_cap / csp_copy_checksum_grid_cap /
//     csp_unpack_checksum_grid_cap / csp_pack_checksum_grid_cap
//                     — tools only: the grid caps of the checksum, copy,
//                       unpack and pack-with-checksum kernels (the patch and
//                       rebase kernels share the unpack kernel's), so tests
//                       reach every loop on tiny data.
//
// Kernel design notes (per /opt/skills/guides/MI355X_MICROARCH.md):
//   - wave64; 256-thread blocks = 4 waves;
//   - the MFMA spin uses v_mfma_f32_32x32x16_bf16 (32768 FLOP/instr,
//     ~32 cyc back-to-back issue per SIMD) with 4 independent
//     accumulators per wave so issue is never dependency-stalled;
//   - the HBM sweep reads+writes float4 (16 B/lane) grid-stride with
//     >=1024 workgroups so all 8 XCDs are saturated;
//   - gfx950-only: built with --offload-arch=gfx950, no other targets.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include "../csrc/csp_io.h"  // exact-length fd writes (header-only, host code)

#include <cstdio>
#include <cstring>
#include <ctime>
#include <algorithm>
#include <mutex>
#include <vector>
#include <utility>

// ---------------------------------------------------------------------------
// Error plumbing
// ---------------------------------------------------------------------------

static thread_local char g_err[512];

static int set_err(const char* what, hipError_t e) {
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return -1;
}

#define HIP_TRY(expr)                                    \
    do {                                                 \
        hipError_t _e = (expr);                          \
        if (_e != hipSuccess) return set_err(#expr, _e); \
    } while (0)

extern "C" const char* csp_last_error() { return g_err; }

// ---------------------------------------------------------------------------
// Kernels
// ---------------------------------------------------------------------------

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// MFMA spin: each wave issues `iters` v_mfma_f32_32x32x16_bf16 across 4
// independent accumulators (issue-rate bound, no dependency stall).
__global__ __launch_bounds__(256) void csp_mfma_spin_kernel(
    float* __restrict__ out, int iters) {
    bf16x8 a, b;
    const int lane = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        a[i] = (__bf16)((lane + i) & 7);
        b[i] = (__bf16)((lane * 3 + i) & 7);
    }
    f32x16 acc0 = {}, acc1 = {}, acc2 = {}, acc3 = {};
    for (int i = 0; i < iters; i += 4) {
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc1, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc2, 0, 0, 0);
        acc3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc3, 0, 0, 0);
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) s += acc0[i] + acc1[i] + acc2[i] + acc3[i];
    if (out && s == -1.0f) out[blockIdx.x] = s;  // never true: defeats DCE only
}

// HBM sweep: grid-stride float4 copy (read 16 B + write 16 B per lane per
// element).  Doubles as the bandwidth probe and the HBM warm-up.
// Template knobs measured on-box (tools: csp_hbm_bench):
//   UNROLL — independent loads in flight per lane (ILP on top of the
//            grid's TLP; HBM latency ~900 cyc wants >1 per lane),
//   NT     — nontemporal load+store (aux=2): a pure streaming copy never
//            re-reads, so bypassing L2 residency avoids evicting it.
template <int UNROLL, bool NT>
__global__ __launch_bounds__(256) void csp_hbm_sweep_t(
    const float4* __restrict__ src, float4* __restrict__ dst, size_t n4) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    // nontemporal builtins need a true vector type, not HIP's float4 class
    typedef float f32x4v __attribute__((ext_vector_type(4)));
    const f32x4v* __restrict__ srcv = reinterpret_cast<const f32x4v*>(src);
    f32x4v* __restrict__ dstv = reinterpret_cast<f32x4v*>(dst);
    for (; i + (UNROLL - 1) * stride < n4; i += UNROLL * stride) {
        f32x4v v[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
            v[u] = NT ? __builtin_nontemporal_load(&srcv[i + u * stride])
                      : srcv[i + u * stride];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            if (NT)
                __builtin_nontemporal_store(v[u], &dstv[i + u * stride]);
            else
                dstv[i + u * stride] = v[u];
        }
    }
    for (; i < n4; i += stride) dst[i] = src[i];
}

using sweep_fn = void (*)(const float4*, float4*, size_t);

static sweep_fn sweep_variant(int variant) {
    switch (variant) {
        case 1: return csp_hbm_sweep_t<4, false>;
        case 2: return csp_hbm_sweep_t<1, true>;
        case 3: return csp_hbm_sweep_t<4, true>;
        case 4: return csp_hbm_sweep_t<8, true>;
        default: return csp_hbm_sweep_t<1, false>;
    }
}

// Default variant for probe/warm-up; selected from on-box measurements
// (profiles/hbm_sweep_variants.md): nontemporal/unroll-1 at 1024
// workgroups (4 per CU), fixed copy direction = 6.0 TB/s, 95% of the
// measured float4-copy ceiling.
static int g_sweep_variant = 2;

extern "C" void csp_set_sweep_variant(int v) { g_sweep_variant = v; }

// One launch of the sweep kernel on the caller's buffers: n4 float4 from src
// to dst (both 16-byte aligned device pointers), `blocks` blocks of 256, on
// the null stream like run_hbm_sweep, synchronised before returning.  variant
// < 0 takes g_sweep_variant, an unknown one falls back to variant 0, both
// through sweep_variant() like the probe: tests check here what the kernel
// behind hbm_bw_gbps copies.  A misaligned pointer or blocks < 1 return -1
// with a message and launch nothing.
extern "C" int csp_hbm_sweep_dev(int variant, const void* src, void* dst, size_t n4,
                                 int blocks) {
    if (reinterpret_cast<uintptr_t>(src) % 16 != 0 || reinterpret_cast<uintptr_t>(dst) % 16 != 0) {
        snprintf(g_err, sizeof(g_err),
                 "csp_hbm_sweep_dev: src %p and dst %p must be 16-byte aligned", src, dst);
        return -1;
    }
    if (blocks < 1) {
        snprintf(g_err, sizeof(g_err), "csp_hbm_sweep_dev: blocks %d is less than 1", blocks);
        return -1;
    }
    sweep_fn kern = sweep_variant(variant < 0 ? g_sweep_variant : variant);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, 0, static_cast<const float4*>(src),
                       static_cast<float4*>(dst), n4);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(0));
    return 0;
}

// ---------------------------------------------------------------------------
// Device / measurement helpers
// ---------------------------------------------------------------------------

extern "C" int csp_device_count() {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        set_err("hipGetDeviceCount", e);
        return -1;
    }
    return n;
}

static int run_mfma_spin(int iters_per_wave, int blocks, float* ms_out) {
    hipEvent_t t0, t1;
    HIP_TRY(hipEventCreate(&t0));
    HIP_TRY(hipEventCreate(&t1));
    HIP_TRY(hipEventRecord(t0));
    hipLaunchKernelGGL(csp_mfma_spin_kernel, dim3(blocks), dim3(256), 0, 0,
                       nullptr, iters_per_wave);
    HIP_TRY(hipEventRecord(t1));
    HIP_TRY(hipEventSynchronize(t1));
    HIP_TRY(hipEventElapsedTime(ms_out, t0, t1));
    HIP_TRY(hipEventDestroy(t0));
    HIP_TRY(hipEventDestroy(t1));
    return 0;
}

static int run_hbm_sweep(float4* buf_a, float4* buf_b, size_t n4, int reps,
                         float* ms_out, int variant = -1, int blocks = 1024,
                         bool pingpong = false) {
    sweep_fn kern = sweep_variant(variant < 0 ? g_sweep_variant : variant);
    hipEvent_t t0, t1;
    HIP_TRY(hipEventCreate(&t0));
    HIP_TRY(hipEventCreate(&t1));
    HIP_TRY(hipEventRecord(t0));
    for (int r = 0; r < reps; ++r) {
        // ping-pong alternates direction; fixed always copies a -> b
        const float4* s = (pingpong && (r & 1)) ? buf_b : buf_a;
        float4* d = (pingpong && (r & 1)) ? buf_a : buf_b;
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, 0, s, d, n4);
    }
    HIP_TRY(hipEventRecord(t1));
    HIP_TRY(hipEventSynchronize(t1));
    HIP_TRY(hipEventElapsedTime(ms_out, t0, t1));
    HIP_TRY(hipEventDestroy(t0));
    HIP_TRY(hipEventDestroy(t1));
    return 0;
}

// FLOP per v_mfma_f32_32x32x16_bf16: 2*32*32*16
static const double kFlopPerMfma = 32768.0;

extern "C" int csp_warmup(int device, int budget_ms) {
    HIP_TRY(hipSetDevice(device));
    if (budget_ms <= 0) budget_ms = 50;
    // One short HBM touch (256 MiB) + an MFMA spin sized to the budget.
    size_t bytes = 256u * 1024u * 1024u;
    size_t n4 = bytes / sizeof(float4);
    float4 *a = nullptr, *b = nullptr;
    HIP_TRY(hipMalloc(&a, bytes));
    HIP_TRY(hipMalloc(&b, bytes));
    HIP_TRY(hipMemsetAsync(a, 1, bytes));
    float ms = 0.f;
    int rc = run_hbm_sweep(a, b, n4, 2, &ms);
    if (rc == 0) {
        // ~40 TFLOP per budget at low clocks -> iters sized for ~budget_ms
        // at an assumed sub-peak 1 PF/s warm-from-idle rate.
        double flops_target = 1.0e12 * (budget_ms / 1000.0) * 2.0;
        int blocks = 1024;
        double waves = (double)blocks * 4.0;
        int iters = (int)(flops_target / (waves * kFlopPerMfma));
        if (iters < 64) iters = 64;
        rc = run_mfma_spin(iters, blocks, &ms);
    }
    (void)hipFree(a);
    (void)hipFree(b);
    return rc;
}

// Properties-only probe: no measurement kernels, no large allocations —
// cheap enough for per-task use (the stub's prologue).  Measured
// bandwidth/TFLOPs fields are 0; csp_probe_json fills them.
extern "C" int csp_probe_props_json(int device, char* buf, size_t buflen) {
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t props;
    HIP_TRY(hipGetDeviceProperties(&props, device));
    size_t mem_free = 0, mem_total = 0;
    HIP_TRY(hipMemGetInfo(&mem_free, &mem_total));
    int written = snprintf(
        buf, buflen,
        "{\"name\":\"%s\",\"gcn_arch\":\"%s\",\"device\":%d,"
        "\"cu_count\":%d,\"max_clock_mhz\":%d,\"lds_per_cu_kb\":%zu,"
        "\"wavefront_size\":%d,\"hbm_total_gb\":%.1f,\"hbm_free_gb\":%.1f,"
        "\"hbm_bw_gbps\":0,\"mfma_bf16_tflops\":0}",
        props.name, props.gcnArchName, device, props.multiProcessorCount,
        props.clockRate / 1000, (size_t)props.maxSharedMemoryPerMultiProcessor / 1024,
        props.warpSize, (double)mem_total / 1.0e9, (double)mem_free / 1.0e9);
    if (written < 0 || (size_t)written >= buflen) {
        snprintf(g_err, sizeof(g_err), "probe json buffer too small");
        return -2;
    }
    return 0;
}

// Lightweight per-task telemetry (worker meta): HBM occupancy without
// the full props query.  One hipMemGetInfo round trip.
extern "C" int csp_mem_info(int device, double* free_gb, double* total_gb) {
    HIP_TRY(hipSetDevice(device));
    size_t mem_free = 0, mem_total = 0;
    HIP_TRY(hipMemGetInfo(&mem_free, &mem_total));
    if (free_gb) *free_gb = (double)mem_free / 1.0e9;
    if (total_gb) *total_gb = (double)mem_total / 1.0e9;
    return 0;
}

extern "C" int csp_probe_json(int device, char* buf, size_t buflen) {
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t props;
    HIP_TRY(hipGetDeviceProperties(&props, device));
    size_t mem_free = 0, mem_total = 0;
    HIP_TRY(hipMemGetInfo(&mem_free, &mem_total));

    // --- measured HBM bandwidth: 1 GiB ping-pong copy ------------------
    size_t bytes = 1024u * 1024u * 1024u;
    size_t n4 = bytes / sizeof(float4);
    float4 *a = nullptr, *b = nullptr;
    HIP_TRY(hipMalloc(&a, bytes));
    HIP_TRY(hipMalloc(&b, bytes));
    HIP_TRY(hipMemsetAsync(a, 1, bytes));
    float warm_ms = 0.f, ms = 0.f;
    int rc = run_hbm_sweep(a, b, n4, 2, &warm_ms);  // warm
    if (rc == 0) rc = run_hbm_sweep(a, b, n4, 6, &ms);
    (void)hipFree(a);
    (void)hipFree(b);
    if (rc != 0) return rc;
    // each rep reads + writes `bytes`
    double hbm_gbps = (2.0 * (double)bytes * 6.0 / 1.0e9) / ((double)ms / 1000.0);

    // --- measured bf16 MFMA throughput ---------------------------------
    const int blocks = 2048;  // 8 WGs/CU; best measured (profiles/)
    const int iters = 8192;   // per wave
    rc = run_mfma_spin(iters / 4, blocks, &warm_ms);  // warm clocks
    if (rc != 0) return rc;
    rc = run_mfma_spin(iters, blocks, &ms);
    if (rc != 0) return rc;
    double waves = (double)blocks * 4.0;
    double tflops = waves * (double)iters * kFlopPerMfma / ((double)ms / 1000.0) / 1.0e12;

    int written = snprintf(
        buf, buflen,
        "{\"name\":\"%s\",\"gcn_arch\":\"%s\",\"device\":%d,"
        "\"cu_count\":%d,\"max_clock_mhz\":%d,\"lds_per_cu_kb\":%zu,"
        "\"wavefront_size\":%d,\"hbm_total_gb\":%.1f,\"hbm_free_gb\":%.1f,"
        "\"hbm_bw_gbps\":%.1f,\"mfma_bf16_tflops\":%.1f}",
        props.name, props.gcnArchName, device, props.multiProcessorCount,
        props.clockRate / 1000, (size_t)props.maxSharedMemoryPerMultiProcessor / 1024,
        props.warpSize, (double)mem_total / 1.0e9, (double)mem_free / 1.0e9,
        hbm_gbps, tflops);
    if (written < 0 || (size_t)written >= buflen) {
        snprintf(g_err, sizeof(g_err), "probe json buffer too small");
        return -2;
    }
    return 0;
}

// ---------------------------------------------------------------------------
// hipHostMalloc-pinned staging
// ---------------------------------------------------------------------------

extern "C" void* csp_host_alloc(size_t nbytes) {
    void* p = nullptr;
    hipError_t e = hipHostMalloc(&p, nbytes, hipHostMallocDefault);
    if (e != hipSuccess) {
        set_err("hipHostMalloc", e);
        return nullptr;
    }
    return p;
}

extern "C" int csp_host_free(void* p) {
    HIP_TRY(hipHostFree(p));
    return 0;
}

// Pooled pinned staging allocator.  A task result may contain several
// large tensors, each needing its own live pinned block until the reply
// is written — so this is a freelist of hipHostMalloc blocks, recycled
// across electrons (pinning 1 GiB costs ~100s of ms; reuse makes it
// one-time).  csp_staging_release_all() returns every outstanding block
// to the freelist; blocks beyond the cache cap are actually freed.
static std::mutex g_staging_mu;
static std::vector<std::pair<void*, size_t>> g_staging_free;
static std::vector<std::pair<void*, size_t>> g_staging_in_use;
static const size_t kStagingCacheCap = size_t(6) << 30;  // 6 GiB pinned cache

extern "C" void* csp_staging_alloc(size_t nbytes) {
    std::lock_guard<std::mutex> lock(g_staging_mu);
    // best-fit from the freelist
    int best = -1;
    for (int i = 0; i < (int)g_staging_free.size(); ++i) {
        if (g_staging_free[i].second >= nbytes &&
            (best < 0 || g_staging_free[i].second < g_staging_free[best].second))
            best = i;
    }
    if (best >= 0) {
        auto blk = g_staging_free[best];
        g_staging_free.erase(g_staging_free.begin() + best);
        g_staging_in_use.push_back(blk);
        return blk.first;
    }
    void* p = nullptr;
    hipError_t e = hipHostMalloc(&p, nbytes, hipHostMallocDefault);
    if (e != hipSuccess) {
        set_err("hipHostMalloc(staging)", e);
        return nullptr;
    }
    g_staging_in_use.push_back({p, nbytes});
    return p;
}

// Back-compat alias (same semantics as alloc).
extern "C" void* csp_staging_get(size_t nbytes) { return csp_staging_alloc(nbytes); }

extern "C" int csp_staging_release_all() {
    std::lock_guard<std::mutex> lock(g_staging_mu);
    for (auto& blk : g_staging_in_use) g_staging_free.push_back(blk);
    g_staging_in_use.clear();
    // trim the cache: keep the largest blocks up to the cap
    std::sort(g_staging_free.begin(), g_staging_free.end(),
              [](auto& a, auto& b) { return a.second > b.second; });
    size_t kept = 0;
    std::vector<std::pair<void*, size_t>> keep;
    for (auto& blk : g_staging_free) {
        if (kept + blk.second <= kStagingCacheCap) {
            kept += blk.second;
            keep.push_back(blk);
        } else {
            HIP_TRY(hipHostFree(blk.first));
        }
    }
    g_staging_free.swap(keep);
    return 0;
}

extern "C" int csp_staging_reset() {
    std::lock_guard<std::mutex> lock(g_staging_mu);
    for (auto& blk : g_staging_free) HIP_TRY(hipHostFree(blk.first));
    for (auto& blk : g_staging_in_use) HIP_TRY(hipHostFree(blk.first));
    g_staging_free.clear();
    g_staging_in_use.clear();
    return 0;
}

// Dedicated copy stream so staging copies never serialize behind the
// caller's compute stream.
static hipStream_t copy_stream() {
    static hipStream_t s = nullptr;
    static std::once_flag once;
    std::call_once(once, [] {
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess)
            s = nullptr;  // fall back to the null stream
    });
    return s;
}

extern "C" int csp_memcpy_d2h(void* dst_host, const void* src_dev, size_t n) {
    hipStream_t s = copy_stream();
    HIP_TRY(hipMemcpyAsync(dst_host, src_dev, n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

extern "C" int csp_memcpy_h2d(void* dst_dev, const void* src_host, size_t n) {
    hipStream_t s = copy_stream();
    HIP_TRY(hipMemcpyAsync(dst_dev, src_host, n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

// Return one block to the staging freelist (the streaming sender's ring;
// csp_staging_release_all would also take back blocks other callers hold).
static void staging_release_one(void* p) {
    if (!p) return;
    std::lock_guard<std::mutex> lock(g_staging_mu);
    for (size_t i = 0; i < g_staging_in_use.size(); ++i) {
        if (g_staging_in_use[i].first == p) {
            g_staging_free.push_back(g_staging_in_use[i]);
            g_staging_in_use.erase(g_staging_in_use.begin() + i);
            return;
        }
    }
}

// ---------------------------------------------------------------------------
// Streaming D2H: one length-framed buffer from device memory to an fd
// ---------------------------------------------------------------------------
//
// Writes the 8-byte big-endian frame length, then the nbytes at src_dev,
// through a ring of two pinned chunks from the staging pool: while chunk
// i is written to fd, the copy of chunk i+1 runs on copy_stream().  The
// D2H engine and the pipe are busy together, and the pinned footprint is
// 2 x chunk_bytes instead of the whole tensor.
//
// Chunk size: sweep over 1/4/16/64 MiB in profiles/staging_return_path.md.
static const size_t kStreamChunkDefault = size_t(16) << 20;
static const int kStreamRing = 2;

#define CSP_STREAM_OK 0
#define CSP_STREAM_FAILED_BEFORE_HEADER 1  // no byte of this frame was written
#define CSP_STREAM_FAILED_MID_FRAME 2      // the frame on fd is cut short

static double mono_ms() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec * 1.0e3 + (double)ts.tv_nsec / 1.0e6;
}

// d2h_ms (optional): copy-engine time summed over the chunks, from events
// around each copy.  write_ms (optional): host time spent inside write().
extern "C" int csp_d2h_stream_fd(int fd, const void* src_dev, size_t nbytes,
                                 size_t chunk_bytes, double* d2h_ms,
                                 double* write_ms) {
    if (d2h_ms) *d2h_ms = 0.0;
    if (write_ms) *write_ms = 0.0;
    if (chunk_bytes == 0) chunk_bytes = kStreamChunkDefault;
    if (chunk_bytes > nbytes) chunk_bytes = nbytes;  // small payload: one short chunk
    const size_t nchunks = nbytes ? (nbytes + chunk_bytes - 1) / chunk_bytes : 0;
    const int ring = nchunks < (size_t)kStreamRing ? (int)nchunks : kStreamRing;

    unsigned char header[8];
    for (int i = 0; i < 8; ++i)
        header[i] = (unsigned char)((unsigned long long)nbytes >> (8 * (7 - i)));

    hipStream_t s = copy_stream();
    void* buf[kStreamRing] = {nullptr, nullptr};
    hipEvent_t ev_start[kStreamRing] = {nullptr, nullptr};
    hipEvent_t ev_done[kStreamRing] = {nullptr, nullptr};
    const char* src = static_cast<const char*>(src_dev);
    bool header_out = false;  // any byte of the header handed to the kernel
    bool copies_issued = false;
    double t_d2h = 0.0, t_write = 0.0;
    int rc = CSP_STREAM_OK;

    auto fail_hip = [&](const char* what, hipError_t e) {
        set_err(what, e);
        rc = header_out ? CSP_STREAM_FAILED_MID_FRAME : CSP_STREAM_FAILED_BEFORE_HEADER;
    };
    auto fail_io = [&](const char* what, int io_rc) {
        snprintf(g_err, sizeof(g_err), "%s: %s", what, strerror(-io_rc));
        rc = header_out ? CSP_STREAM_FAILED_MID_FRAME : CSP_STREAM_FAILED_BEFORE_HEADER;
    };
    auto issue = [&](size_t i) -> bool {
        const int slot = (int)(i % kStreamRing);
        const size_t off = i * chunk_bytes;
        const size_t len = std::min(chunk_bytes, nbytes - off);
        hipError_t e = hipEventRecord(ev_start[slot], s);
        if (e == hipSuccess)
            e = hipMemcpyAsync(buf[slot], src + off, len, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipEventRecord(ev_done[slot], s);
        copies_issued = true;
        if (e != hipSuccess) { fail_hip("stream chunk copy", e); return false; }
        return true;
    };
    auto timed_write = [&](const void* p, size_t n) -> bool {
        size_t done = 0;
        const double t0 = mono_ms();
        int io_rc = csp_io_detail::write_full(fd, p, n, &done);
        t_write += mono_ms() - t0;
        if (done > 0) header_out = true;
        if (io_rc != CSP_IO_OK) { fail_io("stream write", io_rc); return false; }
        return true;
    };

    for (int k = 0; k < ring && rc == CSP_STREAM_OK; ++k) {
        buf[k] = csp_staging_alloc(chunk_bytes);
        if (!buf[k]) { rc = CSP_STREAM_FAILED_BEFORE_HEADER; break; }  // g_err set
        hipError_t e = hipEventCreate(&ev_start[k]);
        if (e == hipSuccess) e = hipEventCreate(&ev_done[k]);
        if (e != hipSuccess) fail_hip("hipEventCreate", e);
    }

    // The first chunk's copy is in flight before the header goes out, so
    // a bad source pointer fails the call before the frame has begun.
    if (rc == CSP_STREAM_OK && nchunks > 0) issue(0);
    if (rc == CSP_STREAM_OK && nchunks > 0) {
        hipError_t e = hipEventSynchronize(ev_done[0]);
        if (e != hipSuccess) fail_hip("hipEventSynchronize", e);
    }
    if (rc == CSP_STREAM_OK) timed_write(header, sizeof(header));

    for (size_t i = 0; i < nchunks && rc == CSP_STREAM_OK; ++i) {
        const int slot = (int)(i % kStreamRing);
        // slot of chunk i+1 held chunk i-1, whose write has returned
        if (i + 1 < nchunks && !issue(i + 1)) break;
        hipError_t e = hipEventSynchronize(ev_done[slot]);
        if (e != hipSuccess) { fail_hip("hipEventSynchronize", e); break; }
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ev_start[slot], ev_done[slot]) == hipSuccess)
            t_d2h += ms;
        const size_t off = i * chunk_bytes;
        if (!timed_write(buf[slot], std::min(chunk_bytes, nbytes - off))) break;
    }

    // No copy may still target a ring buffer once it is back in the pool.
    if (copies_issued && rc != CSP_STREAM_OK) (void)hipStreamSynchronize(s);
    for (int k = 0; k < kStreamRing; ++k) {
        if (ev_start[k]) (void)hipEventDestroy(ev_start[k]);
        if (ev_done[k]) (void)hipEventDestroy(ev_done[k]);
        staging_release_one(buf[k]);
    }
    if (d2h_ms) *d2h_ms = t_d2h;
    if (write_ms) *write_ms = t_write;
    return rc;
}

// ---------------------------------------------------------------------------
// Streaming H2D: one length-framed buffer from an fd into device memory
// ---------------------------------------------------------------------------
//
// The mirror of csp_d2h_stream_fd for tensor ARGUMENTS.  Reads the 8-byte
// big-endian frame length (it must equal nbytes), then the payload chunk by
// chunk into the same two-chunk pinned ring: while chunk i is copied to
// dst_dev on copy_stream(), chunk i+1 is read from fd into the other slot.
// A slot is refilled only after the event behind its last copy has fired.
// Never asks fd for a byte past the frame.
//
// A failure on the request side can still be reported as a task error as
// long as the stream stays aligned, hence three outcomes:
#define CSP_H2D_OK 0              // frame consumed, data on the device
                                  // (dst_dev == nullptr: consumed and discarded)
#define CSP_H2D_FAILED_DRAINED 1  // a HIP call failed; the rest of the frame was
                                  // read and discarded, the stream is aligned
#define CSP_H2D_FAILED_STREAM 2   // EOF, I/O error, timeout or header mismatch:
                                  // the stream is unusable
//
// After the first HIP error no further copy is issued; the call only drains.
// read_ms (optional): host time inside read().  h2d_ms (optional): copy-engine
// time summed over the chunks, from events around each copy.
extern "C" int csp_h2d_stream_fd(int fd, void* dst_dev, size_t nbytes,
                                 size_t chunk_bytes, int timeout_ms,
                                 double* read_ms, double* h2d_ms) {
    if (read_ms) *read_ms = 0.0;
    if (h2d_ms) *h2d_ms = 0.0;
    double t_read = 0.0, t_h2d = 0.0;
    int rc = CSP_H2D_OK;

    auto timed_read = [&](void* p, size_t n) -> bool {
        const double t0 = mono_ms();
        int io_rc = csp_io_detail::read_full(fd, p, n, timeout_ms, nullptr);
        t_read += mono_ms() - t0;
        if (io_rc == CSP_IO_OK) return true;
        if (io_rc == CSP_IO_EOF)
            snprintf(g_err, sizeof(g_err), "stream read: end of file inside the frame");
        else if (io_rc == CSP_IO_TIMEOUT)
            snprintf(g_err, sizeof(g_err), "stream read: timed out");
        else
            snprintf(g_err, sizeof(g_err), "stream read: %s", strerror(-io_rc));
        rc = CSP_H2D_FAILED_STREAM;
        return false;
    };

    unsigned char header[8];
    if (!timed_read(header, sizeof(header))) {
        if (read_ms) *read_ms = t_read;
        return rc;
    }
    unsigned long long announced = 0;
    for (int i = 0; i < 8; ++i) announced = (announced << 8) | header[i];
    if (announced != (unsigned long long)nbytes) {
        snprintf(g_err, sizeof(g_err),
                 "stream header announces %llu bytes, expected %llu", announced,
                 (unsigned long long)nbytes);
        if (read_ms) *read_ms = t_read;
        return CSP_H2D_FAILED_STREAM;
    }

    if (chunk_bytes == 0) chunk_bytes = kStreamChunkDefault;
    if (chunk_bytes > nbytes) chunk_bytes = nbytes;  // small payload: one short chunk
    const size_t nchunks = nbytes ? (nbytes + chunk_bytes - 1) / chunk_bytes : 0;
    const int ring = nchunks < (size_t)kStreamRing ? (int)nchunks : kStreamRing;

    hipStream_t s = copy_stream();
    void* buf[kStreamRing] = {nullptr, nullptr};
    hipEvent_t ev_start[kStreamRing] = {nullptr, nullptr};
    hipEvent_t ev_done[kStreamRing] = {nullptr, nullptr};
    bool in_flight[kStreamRing] = {false, false};  // a copy recorded, not yet timed
    char* dst = static_cast<char*>(dst_dev);
    bool copies_issued = false;
    bool hip_failed = false;  // g_err holds the first HIP error
    size_t consumed = 0;      // payload bytes taken off fd

    auto fail_hip = [&](const char* what, hipError_t e) {
        if (!hip_failed) set_err(what, e);
        hip_failed = true;
    };
    // wait for the copy that last used `slot`, and add its time
    auto retire = [&](int slot) {
        if (!in_flight[slot]) return;
        in_flight[slot] = false;
        hipError_t e = hipEventSynchronize(ev_done[slot]);
        if (e != hipSuccess) { fail_hip("hipEventSynchronize", e); return; }
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ev_start[slot], ev_done[slot]) == hipSuccess)
            t_h2d += ms;
    };

    if (dst) {
        for (int k = 0; k < ring && !hip_failed; ++k) {
            buf[k] = csp_staging_alloc(chunk_bytes);
            if (!buf[k]) { hip_failed = true; break; }  // g_err set
            hipError_t e = hipEventCreate(&ev_start[k]);
            if (e == hipSuccess) e = hipEventCreate(&ev_done[k]);
            if (e != hipSuccess) fail_hip("hipEventCreate", e);
        }
    }

    for (size_t i = 0; dst && i < nchunks && !hip_failed; ++i) {
        const int slot = (int)(i % kStreamRing);
        const size_t off = i * chunk_bytes;
        const size_t len = std::min(chunk_bytes, nbytes - off);
        retire(slot);  // chunk i-2 has left this slot
        if (hip_failed) break;
        if (!timed_read(buf[slot], len)) break;
        consumed += len;
        hipError_t e = hipEventRecord(ev_start[slot], s);
        if (e == hipSuccess)
            e = hipMemcpyAsync(dst + off, buf[slot], len, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipEventRecord(ev_done[slot], s);
        copies_issued = true;
        if (e != hipSuccess) { fail_hip("stream chunk copy", e); break; }
        in_flight[slot] = true;
    }

    // Drain mode, or a HIP failure part-way: take the rest of the frame off
    // fd into plain host memory (the ring may still have copies in flight)
    // so the next frame starts where the peer put it.
    if (rc == CSP_H2D_OK && consumed < nbytes) {
        std::vector<char> scratch(std::min(nbytes - consumed, size_t(1) << 20));
        while (consumed < nbytes) {
            const size_t len = std::min(scratch.size(), nbytes - consumed);
            if (!timed_read(scratch.data(), len)) break;
            consumed += len;
        }
    }

    // No copy may still read a ring buffer once it is back in the pool, and
    // the caller may use dst_dev on any stream after this returns.
    if (copies_issued) {
        hipError_t e = hipStreamSynchronize(s);
        if (e != hipSuccess) fail_hip("hipStreamSynchronize", e);
    }
    for (int k = 0; k < kStreamRing; ++k) {
        if (!hip_failed) retire(k);  // already complete: only adds its time
        if (ev_start[k]) (void)hipEventDestroy(ev_start[k]);
        if (ev_done[k]) (void)hipEventDestroy(ev_done[k]);
        staging_release_one(buf[k]);
    }
    if (read_ms) *read_ms = t_read;
    if (h2d_ms) *h2d_ms = t_h2d;
    if (rc == CSP_H2D_OK && hip_failed) rc = CSP_H2D_FAILED_DRAINED;
    return rc;
}

// ---------------------------------------------------------------------------
// Argument checksum on the device
// ---------------------------------------------------------------------------
//
// The same two numbers as csp_io_detail::checksum (csp_io.h) over bytes that
// are already in HBM: little-endian u32 words w_i, s0 = sum w_i,
// s1 = sum w_i * ((i mod 2^32) + 1), both modulo 2^64.  Integer sums are
// exact in any order, so the block/grid decomposition cannot change them.
//
//   - grid-stride over 16-byte vectors (one global_load_dwordx4 per lane
//     per trip), 256-thread blocks = 4 waves of 64, at most 1024 blocks
//     like the HBM sweep; 4 independent loads in flight per lane;
//   - each lane keeps two u64 accumulators: s0 and t = sum w_i * (i mod
//     2^32), a u32 x u32 -> u64 multiply-add; s1 = t + s0;
//   - wave reduction by shuffles, block reduction through LDS, then one
//     atomicAdd per block and sum on two device u64;
//   - the n mod 16 tail bytes are read one by one by lane 0 of block 0.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
static const int kChecksumUnroll = 4;

__device__ __forceinline__ void checksum_add(unsigned long long& s0,
                                             unsigned long long& t,
                                             u32x4 v, unsigned int word0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        s0 += v[j];
        t += (unsigned long long)v[j] * (unsigned int)(word0 + j);
    }
}

__global__ __launch_bounds__(256) void csp_checksum_kernel(
    const u32x4* __restrict__ src, size_t n16, const unsigned char* __restrict__ tail,
    unsigned int tail_bytes, unsigned long long* __restrict__ out) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long s0 = 0, t = 0;
    for (; i + (kChecksumUnroll - 1) * stride < n16; i += kChecksumUnroll * stride) {
        u32x4 v[kChecksumUnroll];
#pragma unroll
        for (int u = 0; u < kChecksumUnroll; ++u) v[u] = src[i + u * stride];
#pragma unroll
        for (int u = 0; u < kChecksumUnroll; ++u)
            checksum_add(s0, t, v[u], (unsigned int)((i + u * stride) * 4));
    }
    for (; i < n16; i += stride) checksum_add(s0, t, src[i], (unsigned int)(i * 4));

    if (blockIdx.x == 0 && threadIdx.x == 0) {
        for (unsigned int b = 0; b < tail_bytes; ++b) {
            const unsigned long long w = (unsigned long long)tail[b] << (8 * (b & 3));
            s0 += w;
            t += w * (unsigned int)(n16 * 4 + (b >> 2));
        }
    }
    unsigned long long s1 = t + s0;

    for (int off = 32; off > 0; off >>= 1) {
        s0 += __shfl_down(s0, off, 64);
        s1 += __shfl_down(s1, off, 64);
    }
    __shared__ unsigned long long part[2][4];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[0][wave] = s0;
        part[1][wave] = s1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(&out[0], part[0][0] + part[0][1] + part[0][2] + part[0][3]);
        atomicAdd(&out[1], part[1][0] + part[1][1] + part[1][2] + part[1][3]);
    }
}

static std::mutex g_checksum_mu;

static const size_t kChecksumGridCapDefault = 1024;
static size_t g_checksum_grid_cap = kChecksumGridCapDefault;

// Tools only: the grid cap of the next csp_checksum_dev calls (0 restores
// the default).  Returns the cap in effect.  With a cap of 1, 2 or 3 blocks
// a few KiB reach the unrolled loop, the single-vector loop and the hand-off
// between them.
extern "C" size_t csp_checksum_grid_cap(size_t cap) {
    g_checksum_grid_cap = cap ? std::min(cap, size_t(65536)) : kChecksumGridCapDefault;
    return g_checksum_grid_cap;
}

// Checksum of nbytes at device pointer dev (16-byte aligned) into out[2].
// Runs on copy_stream(), so it is ordered after the copies that
// csp_h2d_stream_fd issued, and synchronises that stream before returning.
extern "C" int csp_checksum_dev(const void* dev, size_t nbytes, uint64_t out[2]) {
    out[0] = out[1] = 0;
    if (nbytes == 0) return 0;
    if (reinterpret_cast<uintptr_t>(dev) % 16 != 0) {
        snprintf(g_err, sizeof(g_err),
                 "csp_checksum_dev: device pointer %p is not 16-byte aligned", dev);
        return -1;
    }
    // one accumulator pair per process, one call at a time
    std::lock_guard<std::mutex> lock(g_checksum_mu);
    static unsigned long long* acc = nullptr;
    static int acc_device = -1;
    int device = 0;
    HIP_TRY(hipGetDevice(&device));
    if (acc == nullptr || acc_device != device) {
        if (acc) (void)hipFree(acc);
        acc = nullptr;
        HIP_TRY(hipMalloc(&acc, 2 * sizeof(unsigned long long)));
        acc_device = device;
    }
    const size_t n16 = nbytes / 16;
    const unsigned int tail_bytes = (unsigned int)(nbytes % 16);
    size_t blocks = (n16 + 255) / 256;
    if (blocks < 1) blocks = 1;  // tail only
    if (blocks > g_checksum_grid_cap) blocks = g_checksum_grid_cap;
    hipStream_t s = copy_stream();
    HIP_TRY(hipMemsetAsync(acc, 0, 2 * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(csp_checksum_kernel, dim3((unsigned int)blocks), dim3(256), 0, s,
                       static_cast<const u32x4*>(dev), n16,
                       static_cast<const unsigned char*>(dev) + n16 * 16, tail_bytes,
                       acc);
    HIP_TRY(hipGetLastError());
    unsigned long long host[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(host, acc, sizeof(host), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    out[0] = host[0];
    out[1] = host[1];
    return 0;
}

// ---------------------------------------------------------------------------
// Copy with checksum: a cached argument's private copy, verified on the way
// ---------------------------------------------------------------------------
//
// The worker keeps repeated tensor arguments as master buffers in HBM and
// hands every electron a private copy.  This kernel makes that copy and
// computes csp_checksum_dev's (s0, s1) over the same bytes in ONE pass: one
// HBM read and one write, where clone() followed by csp_checksum_dev reads
// twice and writes once.
//
//   - the checksum kernel's shape: 256-thread blocks, grid-stride over
//     16-byte vectors with 4 independent loads in flight per lane, the same
//     per-lane u64 accumulators, shuffles, LDS, one atomic pair per block;
//   - the loads are plain (the master is read again by the next hit, so it
//     may stay in the caches); the stores are aligned nontemporal 16-byte
//     stores (the copy is not re-read here);
//   - the n mod 16 tail bytes are copied and folded one by one by lane 0 of
//     block 0; no byte at or after src + n is read, none outside
//     [dst, dst + n) is written;
//   - at most 1024 blocks, the checksum kernel's cap: measured against the
//     pack kernel's 2048 it was faster at every size (0.054 against 0.078 ms
//     at 16 MiB, 0.062 against 0.083 ms at 64 MiB, 0.522 against 0.536 ms at
//     1 GiB; profiles/arg_cache.md).
static const size_t kCopyChecksumGridCapDefault = 1024;
static size_t g_copy_checksum_grid_cap = kCopyChecksumGridCapDefault;

// Tools only: the grid cap of the next csp_copy_checksum_dev calls
// (0 restores the default).  Returns the cap in effect.
extern "C" size_t csp_copy_checksum_grid_cap(size_t cap) {
    g_copy_checksum_grid_cap = cap ? std::min(cap, size_t(65536)) : kCopyChecksumGridCapDefault;
    return g_copy_checksum_grid_cap;
}

__global__ __launch_bounds__(256) void csp_copy_checksum_kernel(
    const u32x4* __restrict__ src, u32x4* __restrict__ dst, size_t n16,
    unsigned int tail_bytes, unsigned long long* __restrict__ out) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long s0 = 0, t = 0;
    for (; i + (kChecksumUnroll - 1) * stride < n16; i += kChecksumUnroll * stride) {
        u32x4 v[kChecksumUnroll];
#pragma unroll
        for (int u = 0; u < kChecksumUnroll; ++u) v[u] = src[i + u * stride];
#pragma unroll
        for (int u = 0; u < kChecksumUnroll; ++u) {
            __builtin_nontemporal_store(v[u], &dst[i + u * stride]);
            checksum_add(s0, t, v[u], (unsigned int)((i + u * stride) * 4));
        }
    }
    for (; i < n16; i += stride) {
        const u32x4 v = src[i];
        __builtin_nontemporal_store(v, &dst[i]);
        checksum_add(s0, t, v, (unsigned int)(i * 4));
    }

    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const unsigned char* tail_src = reinterpret_cast<const unsigned char*>(src + n16);
        unsigned char* tail_dst = reinterpret_cast<unsigned char*>(dst + n16);
        for (unsigned int b = 0; b < tail_bytes; ++b) {
            const unsigned char byte = tail_src[b];
            tail_dst[b] = byte;
            const unsigned long long w = (unsigned long long)byte << (8 * (b & 3));
            s0 += w;
            t += w * (unsigned int)(n16 * 4 + (b >> 2));
        }
    }
    unsigned long long s1 = t + s0;

    for (int off = 32; off > 0; off >>= 1) {
        s0 += __shfl_down(s0, off, 64);
        s1 += __shfl_down(s1, off, 64);
    }
    __shared__ unsigned long long part[2][4];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[0][wave] = s0;
        part[1][wave] = s1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(&out[0], part[0][0] + part[0][1] + part[0][2] + part[0][3]);
        atomicAdd(&out[1], part[1][0] + part[1][1] + part[1][2] + part[1][3]);
    }
}

// Copy nbytes from device pointer src to device pointer dst (both 16-byte
// aligned, the ranges disjoint) and put csp_checksum_dev's (s0, s1) of those
// bytes into out[2].  A misaligned pointer or overlapping ranges return -1
// with a message and launch nothing.  Runs on copy_stream(), so it is
// ordered after the copies csp_h2d_stream_fd issued, and synchronises that
// stream before returning; a src written or a dst still in use on another
// stream must be complete first.
extern "C" int csp_copy_checksum_dev(void* dst, const void* src, size_t nbytes,
                                     uint64_t out[2]) {
    out[0] = out[1] = 0;
    if (nbytes == 0) return 0;
    const uintptr_t d = reinterpret_cast<uintptr_t>(dst);
    const uintptr_t s_addr = reinterpret_cast<uintptr_t>(src);
    if (d == 0 || s_addr == 0) {
        snprintf(g_err, sizeof(g_err), "csp_copy_checksum_dev: null pointer for %zu bytes",
                 nbytes);
        return -1;
    }
    if (d % 16 != 0 || s_addr % 16 != 0) {
        snprintf(g_err, sizeof(g_err),
                 "csp_copy_checksum_dev: dst %p and src %p must be 16-byte aligned", dst, src);
        return -1;
    }
    if (d + nbytes < d || s_addr + nbytes < s_addr ||
        (d < s_addr + nbytes && s_addr < d + nbytes)) {
        snprintf(g_err, sizeof(g_err),
                 "csp_copy_checksum_dev: %zu bytes at dst %p and src %p overlap", nbytes, dst,
                 src);
        return -1;
    }
    // one accumulator pair per process, one call at a time
    std::lock_guard<std::mutex> lock(g_checksum_mu);
    static unsigned long long* acc = nullptr;
    static int acc_device = -1;
    int device = 0;
    HIP_TRY(hipGetDevice(&device));
    if (acc == nullptr || acc_device != device) {
        if (acc) (void)hipFree(acc);
        acc = nullptr;
        HIP_TRY(hipMalloc(&acc, 2 * sizeof(unsigned long long)));
        acc_device = device;
    }
    const size_t n16 = nbytes / 16;
    const unsigned int tail_bytes = (unsigned int)(nbytes % 16);
    size_t blocks = (n16 + 255) / 256;
    if (blocks < 1) blocks = 1;  // tail only
    if (blocks > g_copy_checksum_grid_cap) blocks = g_copy_checksum_grid_cap;
    hipStream_t s = copy_stream();
    HIP_TRY(hipMemsetAsync(acc, 0, 2 * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(csp_copy_checksum_kernel, dim3((unsigned int)blocks), dim3(256), 0, s,
                       static_cast<const u32x4*>(src), static_cast<u32x4*>(dst), n16,
                       tail_bytes, acc);
    HIP_TRY(hipGetLastError());
    unsigned long long host[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(host, acc, sizeof(host), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    out[0] = host[0];
    out[1] = host[1];
    return 0;
}

// ---------------------------------------------------------------------------
// Result packing: many small device buffers into one contiguous arena
// ---------------------------------------------------------------------------
//
// A result made of hundreds of small CUDA tensors leaves as ONE streamed,
// checksummed frame: this kernel gathers them into an arena that
// csp_checksum_dev and csp_d2h_stream_fd then treat as one buffer.
//
// Layout (computed by the caller, checked here before anything is launched):
// segment k is nbytes[k] bytes at src[k] and goes to arena + dst_off[k];
// dst_off[0] == 0, dst_off[k+1] == dst_off[k] + round_up(nbytes[k], 16),
// arena_bytes is the sum of the rounded sizes, arena is 16-byte aligned.
// Every arena byte therefore belongs to the 16-byte vectors of exactly one
// segment, and the kernel stores each of those vectors once: the 0..15
// bytes after a segment's data are written as zeros in its last vector.
//
//   - one launch for all segments (multi-tensor style): work is cut into
//     tiles of kPackTileBytes of one segment (256 lanes x 16 B x 4 unrolled
//     trips, the checksum kernel's unroll); the host builds the prefix of
//     tile counts, each block loops over tiles and finds its segment by a
//     binary search that depends on the tile index only (wave-uniform);
//   - 256-thread blocks, grid = min(total tiles, 2048);
//   - a 16-byte aligned source moves with nontemporal 16-byte loads, any
//     other at its own natural alignment (8, 4, 2 or 1 bytes); the stores
//     are always aligned nontemporal 16-byte stores (nothing is re-read);
//   - no byte before src[k] or at or after src[k] + nbytes[k] is read: only
//     vectors wholly inside the segment are loaded whole, the nbytes % 16
//     tail is read byte by byte and merged with zeros.
struct PackSeg {
    const unsigned char* src;
    unsigned long long dst_off;
    unsigned long long nbytes;
    unsigned long long tile_begin;  // tiles owned by the segments before this one
};

static const int kPackUnroll = 4;
static const size_t kPackTileVecs = size_t(256) * kPackUnroll;
static const size_t kPackTileBytes = kPackTileVecs * 16;
static const size_t kPackGridCap = 2048;

typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
typedef unsigned char u8x16 __attribute__((ext_vector_type(16)));

// Sources come out of a table in memory, so the compiler cannot see that
// they are global pointers and would use flat loads: say so.
#define CSP_GLOBAL __attribute__((address_space(1)))
typedef const CSP_GLOBAL unsigned char* pack_src_t;

// 16 bytes at p, which is ALIGN-byte aligned and has 16 readable bytes.
// The source states no more alignment than the pointer has; where the
// compiler fuses the narrow loads into one wider load of the same 16 bytes
// it does so under the target's unaligned-access mode for global memory.
template <int ALIGN>
__device__ __forceinline__ u32x4 pack_load16(pack_src_t p) {
    if constexpr (ALIGN == 16) {
        return __builtin_nontemporal_load(reinterpret_cast<const CSP_GLOBAL u32x4*>(p));
    } else if constexpr (ALIGN == 8) {
        const CSP_GLOBAL unsigned long long* q =
            reinterpret_cast<const CSP_GLOBAL unsigned long long*>(p);
        u64x2 v = {q[0], q[1]};
        return __builtin_bit_cast(u32x4, v);
    } else if constexpr (ALIGN == 4) {
        const CSP_GLOBAL unsigned int* q = reinterpret_cast<const CSP_GLOBAL unsigned int*>(p);
        u32x4 v = {q[0], q[1], q[2], q[3]};
        return v;
    } else if constexpr (ALIGN == 2) {
        const CSP_GLOBAL unsigned short* q =
            reinterpret_cast<const CSP_GLOBAL unsigned short*>(p);
        u16x8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = q[j];
        return __builtin_bit_cast(u32x4, v);
    } else {
        u8x16 v;
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = p[j];
        return __builtin_bit_cast(u32x4, v);
    }
}

// the last `r` (1..15) bytes of a segment, zero-extended to 16
__device__ __forceinline__ u32x4 pack_load_tail(pack_src_t p, unsigned int r) {
    unsigned int w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (unsigned int b = 0; b < 15; ++b)
        if (b < r) w[b >> 2] |= (unsigned int)p[b] << (8 * (b & 3));
    u32x4 v = {w[0], w[1], w[2], w[3]};
    return v;
}

template <int ALIGN>
__device__ __forceinline__ void pack_tile(pack_src_t src, u32x4* __restrict__ dst,
                                          size_t nbytes, size_t tile_in_seg) {
    const size_t nfull = nbytes / 16;  // vectors wholly inside the segment
    const size_t v0 = tile_in_seg * kPackTileVecs + threadIdx.x;
    if ((tile_in_seg + 1) * kPackTileVecs <= nfull) {
        // interior tile: every lane has four whole vectors
        u32x4 v[kPackUnroll];
#pragma unroll
        for (int u = 0; u < kPackUnroll; ++u)
            v[u] = pack_load16<ALIGN>(src + (v0 + u * 256) * 16);
#pragma unroll
        for (int u = 0; u < kPackUnroll; ++u)
            __builtin_nontemporal_store(v[u], &dst[v0 + u * 256]);
        return;
    }
    const unsigned int tail = (unsigned int)(nbytes % 16);
#pragma unroll
    for (int u = 0; u < kPackUnroll; ++u) {
        const size_t vi = v0 + u * 256;
        if (vi < nfull)
            __builtin_nontemporal_store(pack_load16<ALIGN>(src + vi * 16), &dst[vi]);
        else if (vi == nfull && tail != 0)
            __builtin_nontemporal_store(pack_load_tail(src + vi * 16, tail), &dst[vi]);
    }
}

__global__ __launch_bounds__(256) void csp_pack_kernel(
    const PackSeg* __restrict__ segs, unsigned int nseg, size_t total_tiles,
    unsigned char* __restrict__ arena) {
    for (size_t tile = blockIdx.x; tile < total_tiles; tile += gridDim.x) {
        // last segment whose first tile is <= tile (tile_begin is strictly
        // increasing: the host leaves zero-byte segments out of the table)
        unsigned int lo = 0, hi = nseg;
        while (hi - lo > 1) {
            const unsigned int mid = (lo + hi) / 2;
            if (segs[mid].tile_begin <= tile) lo = mid; else hi = mid;
        }
        const PackSeg s = segs[lo];
        u32x4* dst = reinterpret_cast<u32x4*>(arena + s.dst_off);
        const size_t t = tile - s.tile_begin;
        const pack_src_t src = (pack_src_t)s.src;
        const unsigned int a = (unsigned int)(reinterpret_cast<uintptr_t>(s.src) & 15u);
        if (a == 0) pack_tile<16>(src, dst, s.nbytes, t);
        else if ((a & 7u) == 0) pack_tile<8>(src, dst, s.nbytes, t);
        else if ((a & 3u) == 0) pack_tile<4>(src, dst, s.nbytes, t);
        else if ((a & 1u) == 0) pack_tile<2>(src, dst, s.nbytes, t);
        else pack_tile<1>(src, dst, s.nbytes, t);
    }
}

extern "C" size_t csp_pack_tile_bytes() { return kPackTileBytes; }

static std::mutex g_pack_mu;

// Gather nseg device segments into `arena` (layout rule above).  A layout
// violation returns -1 with a message and launches nothing.  Runs on
// copy_stream(), so it is ordered before a csp_checksum_dev or
// csp_d2h_stream_fd of the arena, and synchronises that stream before
// returning; sources written on another stream must be complete first.
// kernel_ms (optional): the kernel alone, from events around the launch.
extern "C" int csp_pack_dev(const void* const* src, const uint64_t* dst_off,
                            const uint64_t* nbytes, size_t nseg, void* arena,
                            size_t arena_bytes, double* kernel_ms) {
    if (kernel_ms) *kernel_ms = 0.0;
    if (reinterpret_cast<uintptr_t>(arena) % 16 != 0) {
        snprintf(g_err, sizeof(g_err),
                 "csp_pack_dev: arena pointer %p is not 16-byte aligned", arena);
        return -1;
    }
    if (nseg >= (size_t(1) << 31)) {
        snprintf(g_err, sizeof(g_err), "csp_pack_dev: %zu segments are too many", nseg);
        return -1;
    }
    std::vector<PackSeg> table;
    table.reserve(nseg);
    uint64_t expect = 0, tiles = 0;
    for (size_t k = 0; k < nseg; ++k) {
        if (dst_off[k] != expect) {
            snprintf(g_err, sizeof(g_err),
                     "csp_pack_dev: dst_off[%zu] is %llu, the layout rule gives %llu", k,
                     (unsigned long long)dst_off[k], (unsigned long long)expect);
            return -1;
        }
        const uint64_t rounded = (nbytes[k] + 15) & ~uint64_t(15);
        if (rounded < nbytes[k] || expect + rounded < expect) {
            snprintf(g_err, sizeof(g_err), "csp_pack_dev: segment %zu overflows", k);
            return -1;
        }
        expect += rounded;
        if (nbytes[k] == 0) continue;  // owns no tile
        if (src[k] == nullptr) {
            snprintf(g_err, sizeof(g_err),
                     "csp_pack_dev: segment %zu has %llu bytes at a null pointer", k,
                     (unsigned long long)nbytes[k]);
            return -1;
        }
        table.push_back({static_cast<const unsigned char*>(src[k]), dst_off[k],
                         nbytes[k], tiles});
        tiles += (rounded + kPackTileBytes - 1) / kPackTileBytes;
    }
    if (expect != (uint64_t)arena_bytes) {
        snprintf(g_err, sizeof(g_err),
                 "csp_pack_dev: arena_bytes is %zu, the segments need %llu", arena_bytes,
                 (unsigned long long)expect);
        return -1;
    }
    if (table.empty()) return 0;
    if (arena == nullptr) {
        snprintf(g_err, sizeof(g_err), "csp_pack_dev: null arena for %zu bytes", arena_bytes);
        return -1;
    }

    // one grow-only table per process, one call at a time
    std::lock_guard<std::mutex> lock(g_pack_mu);
    static PackSeg* dev_table = nullptr;
    static size_t dev_cap = 0;  // entries
    static int dev_device = -1;
    int device = 0;
    HIP_TRY(hipGetDevice(&device));
    if (dev_table == nullptr || dev_device != device || dev_cap < table.size()) {
        if (dev_table) (void)hipFree(dev_table);
        dev_table = nullptr;
        dev_cap = 0;
        size_t cap = 1024;
        while (cap < table.size()) cap *= 2;
        HIP_TRY(hipMalloc(&dev_table, cap * sizeof(PackSeg)));
        dev_cap = cap;
        dev_device = device;
    }
    hipStream_t s = copy_stream();
    hipEvent_t t0 = nullptr, t1 = nullptr;
    if (kernel_ms) {
        HIP_TRY(hipEventCreate(&t0));
        hipError_t e = hipEventCreate(&t1);
        if (e != hipSuccess) {
            (void)hipEventDestroy(t0);
            return set_err("hipEventCreate", e);
        }
    }
    auto done = [&](int rc) {
        if (t0) (void)hipEventDestroy(t0);
        if (t1) (void)hipEventDestroy(t1);
        return rc;
    };
#define PACK_TRY(expr)                                             \
    do {                                                           \
        hipError_t _e = (expr);                                    \
        if (_e != hipSuccess) return done(set_err(#expr, _e));     \
    } while (0)
    // `table` outlives the copy: the stream is synchronised below
    PACK_TRY(hipMemcpyAsync(dev_table, table.data(), table.size() * sizeof(PackSeg),
                            hipMemcpyHostToDevice, s));
    const size_t blocks = tiles < kPackGridCap ? (size_t)tiles : kPackGridCap;
    if (t0) PACK_TRY(hipEventRecord(t0, s));
    hipLaunchKernelGGL(csp_pack_kernel, dim3((unsigned int)blocks), dim3(256), 0, s,
                       dev_table, (unsigned int)table.size(), (size_t)tiles,
                       static_cast<unsigned char*>(arena));
    PACK_TRY(hipGetLastError());
    if (t1) PACK_TRY(hipEventRecord(t1, s));
    PACK_TRY(hipStreamSynchronize(s));
    if (kernel_ms) {
        float ms = 0.f;
        PACK_TRY(hipEventElapsedTime(&ms, t0, t1));
        *kernel_ms = ms;
    }
#undef PACK_TRY
    return done(0);
}

// ---------------------------------------------------------------------------
// Result packing with checksum: gather, master copy and checksum in one pass
// ---------------------------------------------------------------------------
//
// The pack kernel's mirror of csp_unpack_checksum_kernel.  A worker that keeps
// a CUDA result in HBM for reuse as an argument (retain_tensor_results) needs
// the result's bytes in a buffer of its own, 16-byte aligned and laid out as
// an argument arena, and their checksum: csp_pack_dev followed by
// csp_checksum_dev reads the sources once and the arena twice.  This kernel
// reads the sources once and writes the arena once, and the sum comes out of
// the registers the vectors pass through.  One segment is the large-tensor
// case: a copy with checksum from a source of ANY alignment, which
// csp_copy_checksum_dev refuses.
//
//   - csp_pack_kernel's decomposition, unchanged: tiles of kPackTileBytes of
//     one segment, the host-built tile prefix, a binary search per tile that
//     depends on the tile index only (wave-uniform), the source alignment
//     class picked per segment from the pointer bits, pack_load16<ALIGN> and
//     pack_load_tail, 256-thread blocks;
//   - every 16-byte vector a segment owns is assembled once, stored once and
//     added to the checksum kernel's per-lane u64 s0/t accumulators exactly as
//     stored, the last vector with its zero padding included; its arena word
//     index is dst_off/4 + 4*vi modulo 2^32, as checksum_add takes it;
//   - the accumulators are carried across all tiles of a block, then wave
//     shuffles, LDS and one atomicAdd pair per block: the sum is
//     csp_checksum_dev(arena, arena_bytes) whatever the tiling;
//   - no byte outside [src[k], src[k] + nbytes[k]) is read, none outside the
//     arena is written, every arena byte is written exactly once;
//   - stores: plain, see kPackChecksumNtStores below;
//   - grid cap: 1024, see kPackChecksumGridCapDefault below;
//   - 59 VGPRs, no scratch, 8 waves per SIMD (-Rpass-analysis=
//     kernel-resource-usage).
#ifndef CSP_PACK_CHECKSUM_NT_STORES
#define CSP_PACK_CHECKSUM_NT_STORES 0
#endif
// The arena is read again at once by the D2H stream and later by every hit,
// so the stores are plain aligned 16-byte stores.  Measured against
// nontemporal ones (this macro set to 1), the kernel alone: faster on the
// arenas (0.104 against 0.118 ms on the 200-tensor, 295 MB mix, 0.101 against
// 0.110 ms on 66 x 4 MiB), level on one 64 MiB segment (0.044 ms both) and on
// 200 x 4 KiB (0.012 ms both), 1 % slower on one 1 GiB segment (0.372 against
// 0.369 ms); profiles/retained_results.md.
static const bool kPackChecksumNtStores = CSP_PACK_CHECKSUM_NT_STORES != 0;

__device__ __forceinline__ void pack_checksum_store(u32x4 v, u32x4* p) {
    if (kPackChecksumNtStores)
        __builtin_nontemporal_store(v, p);
    else
        *p = v;
}

template <int ALIGN>
__device__ __forceinline__ void pack_checksum_tile(pack_src_t src, u32x4* __restrict__ dst,
                                                   size_t nbytes, size_t tile_in_seg,
                                                   unsigned int word_base,
                                                   unsigned long long& s0,
                                                   unsigned long long& t) {
    const size_t nfull = nbytes / 16;  // vectors wholly inside the segment
    const size_t v0 = tile_in_seg * kPackTileVecs + threadIdx.x;
    if ((tile_in_seg + 1) * kPackTileVecs <= nfull) {
        // interior tile: every lane has four whole vectors
        u32x4 v[kPackUnroll];
#pragma unroll
        for (int u = 0; u < kPackUnroll; ++u)
            v[u] = pack_load16<ALIGN>(src + (v0 + u * 256) * 16);
#pragma unroll
        for (int u = 0; u < kPackUnroll; ++u) {
            const size_t vi = v0 + u * 256;
            pack_checksum_store(v[u], &dst[vi]);
            checksum_add(s0, t, v[u], word_base + (unsigned int)(vi * 4));
        }
        return;
    }
    const unsigned int tail = (unsigned int)(nbytes % 16);
#pragma unroll
    for (int u = 0; u < kPackUnroll; ++u) {
        const size_t vi = v0 + u * 256;
        u32x4 v;
        if (vi < nfull)
            v = pack_load16<ALIGN>(src + vi * 16);
        else if (vi == nfull && tail != 0)
            v = pack_load_tail(src + vi * 16, tail);  // zero padded: summed as stored
        else
            continue;
        pack_checksum_store(v, &dst[vi]);
        checksum_add(s0, t, v, word_base + (unsigned int)(vi * 4));
    }
}

__global__ __launch_bounds__(256) void csp_pack_checksum_kernel(
    const PackSeg* __restrict__ segs, unsigned int nseg, PackSeg only, size_t total_tiles,
    unsigned char* __restrict__ arena, unsigned long long* __restrict__ out) {
    unsigned long long s0 = 0, t = 0;
    for (size_t tile = blockIdx.x; tile < total_tiles; tile += gridDim.x) {
        // last segment whose first tile is <= tile (tile_begin is strictly
        // increasing: the host leaves zero-byte segments out of the table)
        unsigned int lo = 0, hi = nseg;
        while (hi - lo > 1) {
            const unsigned int mid = (lo + hi) / 2;
            if (segs[mid].tile_begin <= tile) lo = mid; else hi = mid;
        }
        // one segment (the large-tensor case) travels as a kernel argument:
        // no table in memory, and the host skips its copy
        const PackSeg s = nseg == 1 ? only : segs[lo];
        u32x4* dst = reinterpret_cast<u32x4*>(arena + s.dst_off);
        const size_t ts = tile - s.tile_begin;
        const pack_src_t src = (pack_src_t)s.src;
        // arena-global index of the segment's first word, modulo 2^32 like
        // csp_checksum_kernel's (unsigned int)(i * 4)
        const unsigned int word_base = (unsigned int)(s.dst_off / 4);
        const unsigned int a = (unsigned int)(reinterpret_cast<uintptr_t>(s.src) & 15u);
        if (a == 0) pack_checksum_tile<16>(src, dst, s.nbytes, ts, word_base, s0, t);
        else if ((a & 7u) == 0) pack_checksum_tile<8>(src, dst, s.nbytes, ts, word_base, s0, t);
        else if ((a & 3u) == 0) pack_checksum_tile<4>(src, dst, s.nbytes, ts, word_base, s0, t);
        else if ((a & 1u) == 0) pack_checksum_tile<2>(src, dst, s.nbytes, ts, word_base, s0, t);
        else pack_checksum_tile<1>(src, dst, s.nbytes, ts, word_base, s0, t);
    }
    unsigned long long s1 = t + s0;

    for (int off = 32; off > 0; off >>= 1) {
        s0 += __shfl_down(s0, off, 64);
        s1 += __shfl_down(s1, off, 64);
    }
    __shared__ unsigned long long part[2][4];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[0][wave] = s0;
        part[1][wave] = s1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(&out[0], part[0][0] + part[0][1] + part[0][2] + part[0][3]);
        atomicAdd(&out[1], part[1][0] + part[1][1] + part[1][2] + part[1][3]);
    }
}

// At most 1024 blocks, the checksum-carrying kernels' cap: measured against
// the pack kernel's 2048 it was faster on the arenas and on one 64 MiB
// segment and level elsewhere (0.104 against 0.111 ms on the 295 MB mix, 0.101
// against 0.110 ms on 66 x 4 MiB, 0.044 against 0.063 ms on 64 MiB, 0.372
// against 0.378 ms on 1 GiB, 0.012 ms both on 200 x 4 KiB;
// profiles/retained_results.md).
static const size_t kPackChecksumGridCapDefault = 1024;
static size_t g_pack_checksum_grid_cap = kPackChecksumGridCapDefault;

// Tools only: the grid cap of the next csp_pack_checksum_dev calls (0 restores
// the default).  Returns the cap in effect.  With a cap of 1, 2 or 3 blocks a
// few dozen tiles make every block loop over several tiles.
extern "C" size_t csp_pack_checksum_grid_cap(size_t cap) {
    g_pack_checksum_grid_cap =
        cap ? std::min(cap, size_t(65536)) : kPackChecksumGridCapDefault;
    return g_pack_checksum_grid_cap;
}

// No arena word index reaches 2^32 below this, so the sum needs no wrap test.
// A condition, not a measurement.
static const uint64_t kPackChecksumMaxBytes = uint64_t(16) << 30;

// Gather nseg device segments into `arena` (csp_pack_dev's layout rule) and
// put csp_checksum_dev(arena, arena_bytes) into out[2], from the same pass.
// Returns -1 with a message and launches nothing for everything csp_pack_dev
// refuses, and for two conditions of its own, checked first: arena_bytes
// above 16 GiB, and a source range [src[k], src[k] + nbytes[k]) that overlaps
// [arena, arena + arena_bytes) (ranges that only touch are fine).  Overlap
// between sources is harmless: they are only read.  arena_bytes == 0 gives
// out = (0, 0).  Runs on copy_stream(), so it is ordered before a
// csp_d2h_stream_fd of the arena, and synchronises that stream before
// returning; sources written on another stream must be complete first.
// kernel_ms (optional): the kernel alone, from events around the launch.
extern "C" int csp_pack_checksum_dev(const void* const* src, const uint64_t* dst_off,
                                     const uint64_t* nbytes, size_t nseg, void* arena,
                                     size_t arena_bytes, uint64_t out[2], double* kernel_ms) {
    out[0] = out[1] = 0;
    if (kernel_ms) *kernel_ms = 0.0;
    if ((uint64_t)arena_bytes > kPackChecksumMaxBytes) {
        snprintf(g_err, sizeof(g_err),
                 "csp_pack_checksum_dev: arena_bytes %zu is above 16 GiB", arena_bytes);
        return -1;
    }
    if (nseg >= (size_t(1) << 31)) {  // before anything walks the segments
        snprintf(g_err, sizeof(g_err), "csp_pack_checksum_dev: %zu segments are too many",
                 nseg);
        return -1;
    }
    const uintptr_t a = reinterpret_cast<uintptr_t>(arena);
    if (a + arena_bytes < a) {
        snprintf(g_err, sizeof(g_err),
                 "csp_pack_checksum_dev: %zu bytes at arena %p overflow", arena_bytes, arena);
        return -1;
    }
    for (size_t k = 0; k < nseg; ++k) {
        const uintptr_t p = reinterpret_cast<uintptr_t>(src[k]);
        if (nbytes[k] == 0 || p == 0) continue;  // a null source is refused below
        if (p + nbytes[k] < p) {
            snprintf(g_err, sizeof(g_err),
                     "csp_pack_checksum_dev: src[%zu] %p with %llu bytes overflows", k, src[k],
                     (unsigned long long)nbytes[k]);
            return -1;
        }
        if (p < a + arena_bytes && a < p + nbytes[k]) {
            snprintf(g_err, sizeof(g_err),
                     "csp_pack_checksum_dev: %llu bytes at src[%zu] %p overlap the arena at %p",
                     (unsigned long long)nbytes[k], k, src[k], arena);
            return -1;
        }
    }
    if (a % 16 != 0) {
        snprintf(g_err, sizeof(g_err),
                 "csp_pack_checksum_dev: arena pointer %p is not 16-byte aligned", arena);
        return -1;
    }
    std::vector<PackSeg> table;
    table.reserve(nseg);
    uint64_t expect = 0, tiles = 0;
    for (size_t k = 0; k < nseg; ++k) {
        if (dst_off[k] != expect) {
            snprintf(g_err, sizeof(g_err),
                     "csp_pack_checksum_dev: dst_off[%zu] is %llu, the layout rule gives %llu",
                     k, (unsigned long long)dst_off[k], (unsigned long long)expect);
            return -1;
        }
        const uint64_t rounded = (nbytes[k] + 15) & ~uint64_t(15);
        if (rounded < nbytes[k] || expect + rounded < expect) {
            snprintf(g_err, sizeof(g_err), "csp_pack_checksum_dev: segment %zu overflows", k);
            return -1;
        }
        expect += rounded;
        if (nbytes[k] == 0) continue;  // owns no tile
        if (src[k] == nullptr) {
            snprintf(g_err, sizeof(g_err),
                     "csp_pack_checksum_dev: segment %zu has %llu bytes at a null pointer", k,
                     (unsigned long long)nbytes[k]);
            return -1;
        }
        table.push_back({static_cast<const unsigned char*>(src[k]), dst_off[k],
                         nbytes[k], tiles});
        tiles += (rounded + kPackTileBytes - 1) / kPackTileBytes;
    }
    if (expect != (uint64_t)arena_bytes) {
        snprintf(g_err, sizeof(g_err),
                 "csp_pack_checksum_dev: arena_bytes is %zu, the segments need %llu",
                 arena_bytes, (unsigned long long)expect);
        return -1;
    }
    if (table.empty()) return 0;
    if (arena == nullptr) {
        snprintf(g_err, sizeof(g_err), "csp_pack_checksum_dev: null arena for %zu bytes",
                 arena_bytes);
        return -1;
    }

    // one accumulator pair and one grow-only table per process, one call at
    // a time
    std::lock_guard<std::mutex> lock(g_checksum_mu);
    static unsigned long long* acc = nullptr;
    static PackSeg* dev_table = nullptr;
    static size_t dev_cap = 0;  // entries
    static int dev_device = -1;
    int device = 0;
    HIP_TRY(hipGetDevice(&device));
    if (dev_device != device) {
        if (acc) (void)hipFree(acc);
        if (dev_table) (void)hipFree(dev_table);
        acc = nullptr;
        dev_table = nullptr;
        dev_cap = 0;
        dev_device = device;
    }
    if (acc == nullptr) HIP_TRY(hipMalloc(&acc, 2 * sizeof(unsigned long long)));
    const bool single = table.size() == 1;  // passed by value, see the kernel
    if (!single && (dev_table == nullptr || dev_cap < table.size())) {
        if (dev_table) (void)hipFree(dev_table);
        dev_table = nullptr;
        dev_cap = 0;
        size_t cap = 1024;
        while (cap < table.size()) cap *= 2;
        HIP_TRY(hipMalloc(&dev_table, cap * sizeof(PackSeg)));
        dev_cap = cap;
    }
    hipStream_t s = copy_stream();
    hipEvent_t t0 = nullptr, t1 = nullptr;
    if (kernel_ms) {
        HIP_TRY(hipEventCreate(&t0));
        hipError_t e = hipEventCreate(&t1);
        if (e != hipSuccess) {
            (void)hipEventDestroy(t0);
            return set_err("hipEventCreate", e);
        }
    }
    auto done = [&](int rc) {
        if (t0) (void)hipEventDestroy(t0);
        if (t1) (void)hipEventDestroy(t1);
        return rc;
    };
#define PACKSUM_TRY(expr)                                          \
    do {                                                           \
        hipError_t _e = (expr);                                    \
        if (_e != hipSuccess) return done(set_err(#expr, _e));     \
    } while (0)
    // `table` outlives the copy: the stream is synchronised below
    if (!single)
        PACKSUM_TRY(hipMemcpyAsync(dev_table, table.data(), table.size() * sizeof(PackSeg),
                                   hipMemcpyHostToDevice, s));
    PACKSUM_TRY(hipMemsetAsync(acc, 0, 2 * sizeof(unsigned long long), s));
    const size_t blocks =
        tiles < g_pack_checksum_grid_cap ? (size_t)tiles : g_pack_checksum_grid_cap;
    if (t0) PACKSUM_TRY(hipEventRecord(t0, s));
    hipLaunchKernelGGL(csp_pack_checksum_kernel, dim3((unsigned int)blocks), dim3(256), 0, s,
                       single ? nullptr : dev_table, (unsigned int)table.size(), table[0],
                       (size_t)tiles, static_cast<unsigned char*>(arena), acc);
    PACKSUM_TRY(hipGetLastError());
    if (t1) PACKSUM_TRY(hipEventRecord(t1, s));
    unsigned long long host[2] = {0, 0};
    PACKSUM_TRY(hipMemcpyAsync(host, acc, sizeof(host), hipMemcpyDeviceToHost, s));
    PACKSUM_TRY(hipStreamSynchronize(s));
    if (kernel_ms) {
        float ms = 0.f;
        PACKSUM_TRY(hipEventElapsedTime(&ms, t0, t1));
        *kernel_ms = ms;
    }
#undef PACKSUM_TRY
    out[0] = host[0];
    out[1] = host[1];
    return done(0);
}

// ---------------------------------------------------------------------------
// Argument unpacking: one arena scattered into many private buffers, verified
// ---------------------------------------------------------------------------
//
// The argument-direction mirror of csp_pack_dev.  The small tensor arguments
// of one electron arrive as ONE frame that lands in HBM as one arena (the
// pack layout); this kernel scatters the arena into the electron's private
// per-tensor allocations and computes csp_checksum_dev's (s0, s1) of the
// whole arena in the same pass.  Verification has to read every arena byte
// anyway, so the scatter costs only the writes.
//
// Layout (the pack layout read backwards, checked before anything is
// launched): segment k is nbytes[k] bytes at arena + src_off[k] and goes to
// dst[k]; src_off[0] == 0, src_off[k+1] == src_off[k] + round_up(nbytes[k],
// 16), arena_bytes is the sum of the rounded sizes, arena and every dst are
// 16-byte aligned.  Every 16-byte arena vector belongs to exactly one
// segment and is loaded and summed exactly once, padding included and summed
// as it is (not assumed zero), with word weights from the arena-global word
// index src_off[k]/4 + i: the result is csp_checksum_dev(arena, arena_bytes)
// whatever the tiling, because integer sums are exact in any order.
//
//   - the pack kernel's decomposition: tiles of kPackTileBytes of one
//     segment, the prefix of tile counts built on the host, a binary search
//     per tile that depends on the tile index only (wave-uniform); each block
//     loops over tiles blockIdx.x, +gridDim.x, ... and carries the checksum
//     kernel's per-lane u64 s0/t accumulators across all of them, then wave
//     shuffles, LDS and one atomicAdd pair per block;
//   - arena loads are aligned plain 16-byte loads (a cached master is read
//     again by the next hit, so it may stay in the caches); stores of vectors
//     wholly inside a segment are aligned nontemporal 16-byte stores;
//   - the last vector of a segment with nbytes % 16 != 0 is loaded and summed
//     whole, but only its nbytes % 16 data bytes are stored: dst is 16-byte
//     aligned, so they go out as naturally aligned 8/4/2/1-byte stores picked
//     by the bits of the remainder.  No byte at or after dst[k] + nbytes[k]
//     is written, and no arena byte is written at all;
//   - at most 1024 blocks, the checksum kernels' cap: measured against the
//     pack kernel's 2048 it was faster on the 200-tensor mix and level on
//     the other two layouts (0.0958 against 0.1021 ms on 295 MB, 0.0948 against
//     0.0953 ms on 66 x 4 MiB, 0.0116 ms both on 200 x 4 KiB;
//     profiles/packed_args.md).
struct UnpackSeg {
    unsigned char* dst;
    unsigned long long src_off;
    unsigned long long nbytes;
    unsigned long long tile_begin;  // tiles owned by the segments before this one
};

typedef CSP_GLOBAL unsigned char* unpack_dst_t;

// the first `r` (1..15) bytes of v to the 16-byte aligned p, nothing after
__device__ __forceinline__ void unpack_store_tail(unpack_dst_t p, u32x4 v, unsigned int r) {
    unsigned int pos = 0;
    if (r & 8u) {
        *reinterpret_cast<CSP_GLOBAL unsigned long long*>(p) =
            (unsigned long long)v[0] | ((unsigned long long)v[1] << 32);
        pos = 8;
    }
    if (r & 4u) {
        // pos is 0 or 8: word 0 or word 2
        *reinterpret_cast<CSP_GLOBAL unsigned int*>(p + pos) = pos ? v[2] : v[0];
        pos += 4;
    }
    // the word that holds the remaining 0..3 bytes
    const unsigned int w = pos >= 8 ? (pos >= 12 ? v[3] : v[2]) : (pos >= 4 ? v[1] : v[0]);
    if (r & 2u) {
        *reinterpret_cast<CSP_GLOBAL unsigned short*>(p + pos) = (unsigned short)(w & 0xffffu);
        pos += 2;
    }
    if (r & 1u) p[pos] = (unsigned char)((w >> (8 * (pos & 3u))) & 0xffu);
}

__global__ __launch_bounds__(256) void csp_unpack_checksum_kernel(
    const UnpackSeg* __restrict__ segs, unsigned int nseg, size_t total_tiles,
    const unsigned char* __restrict__ arena, unsigned long long* __restrict__ out) {
    unsigned long long s0 = 0, t = 0;
    for (size_t tile = blockIdx.x; tile < total_tiles; tile += gridDim.x) {
        // last segment whose first tile is <= tile (tile_begin is strictly
        // increasing: the host leaves zero-byte segments out of the table)
        unsigned int lo = 0, hi = nseg;
        while (hi - lo > 1) {
            const unsigned int mid = (lo + hi) / 2;
            if (segs[mid].tile_begin <= tile) lo = mid; else hi = mid;
        }
        const UnpackSeg s = segs[lo];
        const u32x4* __restrict__ src = reinterpret_cast<const u32x4*>(arena + s.src_off);
        const unpack_dst_t dst = (unpack_dst_t)s.dst;
        const size_t nfull = s.nbytes / 16;  // vectors wholly inside the segment
        const unsigned int tail = (unsigned int)(s.nbytes % 16);
        const size_t nvec = nfull + (tail ? 1 : 0);  // vectors the segment owns
        const size_t v0 = (tile - s.tile_begin) * kPackTileVecs + threadIdx.x;
        // arena-global index of the segment's first word, modulo 2^32 like
        // csp_checksum_kernel's (unsigned int)(i * 4)
        const unsigned int word_base = (unsigned int)(s.src_off / 4);
        if ((tile - s.tile_begin + 1) * kPackTileVecs <= nfull) {
            // interior tile: every lane has four whole vectors
            u32x4 v[kPackUnroll];
#pragma unroll
            for (int u = 0; u < kPackUnroll; ++u) v[u] = src[v0 + u * 256];
#pragma unroll
            for (int u = 0; u < kPackUnroll; ++u) {
                const size_t vi = v0 + u * 256;
                __builtin_nontemporal_store(
                    v[u], reinterpret_cast<CSP_GLOBAL u32x4*>(dst + vi * 16));
                checksum_add(s0, t, v[u], word_base + (unsigned int)(vi * 4));
            }
            continue;
        }
#pragma unroll
        for (int u = 0; u < kPackUnroll; ++u) {
            const size_t vi = v0 + u * 256;
            if (vi >= nvec) continue;
            const u32x4 v = src[vi];  // padding included: all 16 bytes are arena
            checksum_add(s0, t, v, word_base + (unsigned int)(vi * 4));
            if (vi < nfull)
                __builtin_nontemporal_store(
                    v, reinterpret_cast<CSP_GLOBAL u32x4*>(dst + vi * 16));
            else
                unpack_store_tail(dst + vi * 16, v, tail);
        }
    }
    unsigned long long s1 = t + s0;

    for (int off = 32; off > 0; off >>= 1) {
        s0 += __shfl_down(s0, off, 64);
        s1 += __shfl_down(s1, off, 64);
    }
    __shared__ unsigned long long part[2][4];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[0][wave] = s0;
        part[1][wave] = s1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(&out[0], part[0][0] + part[0][1] + part[0][2] + part[0][3]);
        atomicAdd(&out[1], part[1][0] + part[1][1] + part[1][2] + part[1][3]);
    }
}

static const size_t kUnpackGridCapDefault = 1024;
static size_t g_unpack_grid_cap = kUnpackGridCapDefault;

// Tools only: the grid cap of the next csp_unpack_checksum_dev calls
// (0 restores the default).  Returns the cap in effect.  With a cap of 1, 2
// or 3 blocks a few dozen tiles make every block loop over several tiles.
extern "C" size_t csp_unpack_checksum_grid_cap(size_t cap) {
    g_unpack_grid_cap = cap ? std::min(cap, size_t(65536)) : kUnpackGridCapDefault;
    return g_unpack_grid_cap;
}

// Scatter the arena's nseg segments to dst[k] (layout rule above) and put
// csp_checksum_dev(arena, arena_bytes) into out[2].  Returns -1 with a
// message and launches nothing for: a misaligned arena, a non-null dst that
// is not 16-byte aligned, a nonzero segment with a null dst, a null arena
// for a nonzero arena_bytes, a layout violation, an arena_bytes that is not
// the layout's total, an overflow, nseg >= 2^31, or a destination range
// [dst[k], dst[k] + nbytes[k]) that overlaps the arena.  Overlap BETWEEN
// destinations is not checked: it is the caller's responsibility, and two
// overlapping destinations end with unspecified bytes where they overlap.
// Zero-byte segments own no tile and their dst may be null.  arena_bytes == 0
// gives out = (0, 0).  Runs on copy_stream(), so it is ordered after the
// copies csp_h2d_stream_fd issued, and synchronises that stream before
// returning; destinations in use on another stream must be complete first.
// kernel_ms (optional): the kernel alone, from events around the launch.
extern "C" int csp_unpack_checksum_dev(const void* arena, size_t arena_bytes,
                                       void* const* dst, const uint64_t* src_off,
                                       const uint64_t* nbytes, size_t nseg,
                                       uint64_t out[2], double* kernel_ms) {
    out[0] = out[1] = 0;
    if (kernel_ms) *kernel_ms = 0.0;
    const uintptr_t a = reinterpret_cast<uintptr_t>(arena);
    if (a % 16 != 0) {
        snprintf(g_err, sizeof(g_err),
                 "csp_unpack_checksum_dev: arena pointer %p is not 16-byte aligned", arena);
        return -1;
    }
    if (nseg >= (size_t(1) << 31)) {
        snprintf(g_err, sizeof(g_err), "csp_unpack_checksum_dev: %zu segments are too many",
                 nseg);
        return -1;
    }
    if (a + arena_bytes < a) {
        snprintf(g_err, sizeof(g_err),
                 "csp_unpack_checksum_dev: %zu bytes at arena %p overflow", arena_bytes, arena);
        return -1;
    }
    std::vector<UnpackSeg> table;
    table.reserve(nseg);
    uint64_t expect = 0, tiles = 0;
    for (size_t k = 0; k < nseg; ++k) {
        if (src_off[k] != expect) {
            snprintf(g_err, sizeof(g_err),
                     "csp_unpack_checksum_dev: src_off[%zu] is %llu, the layout rule gives %llu",
                     k, (unsigned long long)src_off[k], (unsigned long long)expect);
            return -1;
        }
        const uint64_t rounded = (nbytes[k] + 15) & ~uint64_t(15);
        if (rounded < nbytes[k] || expect + rounded < expect) {
            snprintf(g_err, sizeof(g_err), "csp_unpack_checksum_dev: segment %zu overflows", k);
            return -1;
        }
        expect += rounded;
        const uintptr_t d = reinterpret_cast<uintptr_t>(dst[k]);
        if (d % 16 != 0) {
            snprintf(g_err, sizeof(g_err),
                     "csp_unpack_checksum_dev: dst[%zu] %p is not 16-byte aligned", k, dst[k]);
            return -1;
        }
        if (nbytes[k] == 0) continue;  // owns no tile
        if (d == 0) {
            snprintf(g_err, sizeof(g_err),
                     "csp_unpack_checksum_dev: segment %zu has %llu bytes and a null dst", k,
                     (unsigned long long)nbytes[k]);
            return -1;
        }
        if (d + nbytes[k] < d) {
            snprintf(g_err, sizeof(g_err),
                     "csp_unpack_checksum_dev: dst[%zu] %p with %llu bytes overflows", k, dst[k],
                     (unsigned long long)nbytes[k]);
            return -1;
        }
        table.push_back({static_cast<unsigned char*>(dst[k]), src_off[k], nbytes[k], tiles});
        tiles += (rounded + kPackTileBytes - 1) / kPackTileBytes;
    }
    if (expect != (uint64_t)arena_bytes) {
        snprintf(g_err, sizeof(g_err),
                 "csp_unpack_checksum_dev: arena_bytes is %zu, the segments need %llu",
                 arena_bytes, (unsigned long long)expect);
        return -1;
    }
    if (arena_bytes == 0) return 0;
    if (arena == nullptr) {
        snprintf(g_err, sizeof(g_err), "csp_unpack_checksum_dev: null arena for %zu bytes",
                 arena_bytes);
        return -1;
    }
    for (size_t k = 0; k < table.size(); ++k) {
        const uintptr_t d = reinterpret_cast<uintptr_t>(table[k].dst);
        if (d < a + arena_bytes && a < d + table[k].nbytes) {
            snprintf(g_err, sizeof(g_err),
                     "csp_unpack_checksum_dev: %llu bytes at dst %p overlap the arena at %p",
                     (unsigned long long)table[k].nbytes, (void*)table[k].dst, arena);
            return -1;
        }
    }

    // one accumulator pair and one grow-only table per process, one call at
    // a time
    std::lock_guard<std::mutex> lock(g_checksum_mu);
    static unsigned long long* acc = nullptr;
    static UnpackSeg* dev_table = nullptr;
    static size_t dev_cap = 0;  // entries
    static int dev_device = -1;
    int device = 0;
    HIP_TRY(hipGetDevice(&device));
    if (dev_device != device) {
        if (acc) (void)hipFree(acc);
        if (dev_table) (void)hipFree(dev_table);
        acc = nullptr;
        dev_table = nullptr;
        dev_cap = 0;
        dev_device = device;
    }
    if (acc == nullptr) HIP_TRY(hipMalloc(&acc, 2 * sizeof(unsigned long long)));
    if (dev_table == nullptr || dev_cap < table.size()) {
        if (dev_table) (void)hipFree(dev_table);
        dev_table = nullptr;
        dev_cap = 0;
        size_t cap = 1024;
        while (cap < table.size()) cap *= 2;
        HIP_TRY(hipMalloc(&dev_table, cap * sizeof(UnpackSeg)));
        dev_cap = cap;
    }
    hipStream_t s = copy_stream();
    hipEvent_t t0 = nullptr, t1 = nullptr;
    if (kernel_ms) {
        HIP_TRY(hipEventCreate(&t0));
        hipError_t e = hipEventCreate(&t1);
        if (e != hipSuccess) {
            (void)hipEventDestroy(t0);
            return set_err("hipEventCreate", e);
        }
    }
    auto done = [&](int rc) {
        if (t0) (void)hipEventDestroy(t0);
        if (t1) (void)hipEventDestroy(t1);
        return rc;
    };
#define UNPACK_TRY(expr)                                           \
    do {                                                           \
        hipError_t _e = (expr);                                    \
        if (_e != hipSuccess) return done(set_err(#expr, _e));     \
    } while (0)
    // `table` outlives the copy: the stream is synchronised below
    UNPACK_TRY(hipMemcpyAsync(dev_table, table.data(), table.size() * sizeof(UnpackSeg),
                              hipMemcpyHostToDevice, s));
    UNPACK_TRY(hipMemsetAsync(acc, 0, 2 * sizeof(unsigned long long), s));
    const size_t blocks = tiles < g_unpack_grid_cap ? (size_t)tiles : g_unpack_grid_cap;
    if (t0) UNPACK_TRY(hipEventRecord(t0, s));
    hipLaunchKernelGGL(csp_unpack_checksum_kernel, dim3((unsigned int)blocks), dim3(256), 0, s,
                       dev_table, (unsigned int)table.size(), (size_t)tiles,
                       static_cast<const unsigned char*>(arena), acc);
    UNPACK_TRY(hipGetLastError());
    if (t1) UNPACK_TRY(hipEventRecord(t1, s));
    unsigned long long host[2] = {0, 0};
    UNPACK_TRY(hipMemcpyAsync(host, acc, sizeof(host), hipMemcpyDeviceToHost, s));
    UNPACK_TRY(hipStreamSynchronize(s));
    if (kernel_ms) {
        float ms = 0.f;
        UNPACK_TRY(hipEventElapsedTime(&ms, t0, t1));
        *kernel_ms = ms;
    }
#undef UNPACK_TRY
    out[0] = host[0];
    out[1] = host[1];
    return done(0);
}

// ---------------------------------------------------------------------------
// Argument patching: a cached arena updated in place, unpacked and verified
// ---------------------------------------------------------------------------
//
// A cached packed arena (the master) of which only a few segments changed is
// not sent again: the changed segments arrive as a small delta arena, and this
// kernel, in the ONE pass that csp_unpack_checksum_dev makes anyway, writes
// them over the master, scatters the whole new arena into the electron's
// private buffers and computes csp_checksum_dev's (s0, s1) of the master as it
// is afterwards.
//
// Layout: master, src_off, nbytes, dst and arena_bytes follow the unpack
// layout rule above.  delta_off[k] == UINT64_MAX: segment k is unchanged.
// Otherwise its new bytes are at delta + delta_off[k]; the patched segments,
// in segment order, obey the pack layout inside the delta (the first at 0,
// each next one at the previous offset plus round_up(nbytes, 16)), and
// delta_bytes is that total.
//
//   - the unpack kernel's decomposition, unchanged: tiles of kPackTileBytes
//     of one segment, the host-built tile prefix, a binary search per tile
//     that depends on the tile index only, per-lane u64 s0/t accumulators
//     carried across a block's tiles, wave shuffles, LDS, one atomicAdd pair
//     per block, 256-thread blocks, the unpack kernel's grid cap (its 1024 is
//     taken over, not measured for this kernel);
//   - the table entry gains the patch source (null: unchanged), so the choice
//     of source is per tile and wave-uniform;
//   - an unchanged segment takes exactly the unpack path: plain aligned
//     16-byte loads from the master, nontemporal stores to dst, the tail as
//     aligned 8/4/2/1-byte pieces; nothing is written to the master;
//   - a patched segment loads every 16-byte vector it owns from the delta
//     (read once: nontemporal), stores it whole to the master with a plain
//     aligned 16-byte store (the master is re-read by the next hit; the
//     padding of the last vector goes in as the delta has it), stores it to
//     dst by the unpack rules and sums it with the master-global word index;
//   - the delta is never written, no master byte outside a patched segment's
//     vectors is written, and a patched segment is never read from the
//     master, so no lane reads what another writes inside the launch.
struct PatchSeg {
    unsigned char* dst;
    const unsigned char* patch;  // the segment's new bytes in the delta, or null
    unsigned long long src_off;
    unsigned long long nbytes;
    unsigned long long tile_begin;  // tiles owned by the segments before this one
};

__global__ __launch_bounds__(256) void csp_patch_unpack_checksum_kernel(
    const PatchSeg* __restrict__ segs, unsigned int nseg, size_t total_tiles,
    unsigned char* master, unsigned long long* __restrict__ out) {
    unsigned long long s0 = 0, t = 0;
    for (size_t tile = blockIdx.x; tile < total_tiles; tile += gridDim.x) {
        // last segment whose first tile is <= tile (tile_begin is strictly
        // increasing: the host leaves zero-byte segments out of the table)
        unsigned int lo = 0, hi = nseg;
        while (hi - lo > 1) {
            const unsigned int mid = (lo + hi) / 2;
            if (segs[mid].tile_begin <= tile) lo = mid; else hi = mid;
        }
        const PatchSeg s = segs[lo];
        CSP_GLOBAL u32x4* mst = reinterpret_cast<CSP_GLOBAL u32x4*>(
            (CSP_GLOBAL unsigned char*)(master + s.src_off));
        const CSP_GLOBAL u32x4* patch = reinterpret_cast<const CSP_GLOBAL u32x4*>(
            (const CSP_GLOBAL unsigned char*)s.patch);
        const bool patched = s.patch != nullptr;  // per tile: wave-uniform
        const unpack_dst_t dst = (unpack_dst_t)s.dst;
        const size_t nfull = s.nbytes / 16;  // vectors wholly inside the segment
        const unsigned int tail = (unsigned int)(s.nbytes % 16);
        const size_t nvec = nfull + (tail ? 1 : 0);  // vectors the segment owns
        const size_t v0 = (tile - s.tile_begin) * kPackTileVecs + threadIdx.x;
        // master-global index of the segment's first word, modulo 2^32 like
        // csp_checksum_kernel's (unsigned int)(i * 4)
        const unsigned int word_base = (unsigned int)(s.src_off / 4);
        if ((tile - s.tile_begin + 1) * kPackTileVecs <= nfull) {
            // interior tile: every lane has four whole vectors
            u32x4 v[kPackUnroll];
            if (patched) {
#pragma unroll
                for (int u = 0; u < kPackUnroll; ++u)
                    v[u] = __builtin_nontemporal_load(&patch[v0 + u * 256]);
#pragma unroll
                for (int u = 0; u < kPackUnroll; ++u) mst[v0 + u * 256] = v[u];
            } else {
#pragma unroll
                for (int u = 0; u < kPackUnroll; ++u) v[u] = mst[v0 + u * 256];
            }
#pragma unroll
            for (int u = 0; u < kPackUnroll; ++u) {
                const size_t vi = v0 + u * 256;
                __builtin_nontemporal_store(
                    v[u], reinterpret_cast<CSP_GLOBAL u32x4*>(dst + vi * 16));
                checksum_add(s0, t, v[u], word_base + (unsigned int)(vi * 4));
            }
            continue;
        }
#pragma unroll
        for (int u = 0; u < kPackUnroll; ++u) {
            const size_t vi = v0 + u * 256;
            if (vi >= nvec) continue;
            u32x4 v;  // padding included: all 16 bytes are delta or master
            if (patched) {
                v = __builtin_nontemporal_load(&patch[vi]);
                mst[vi] = v;
            } else {
                v = mst[vi];
            }
            checksum_add(s0, t, v, word_base + (unsigned int)(vi * 4));
            if (vi < nfull)
                __builtin_nontemporal_store(
                    v, reinterpret_cast<CSP_GLOBAL u32x4*>(dst + vi * 16));
            else
                unpack_store_tail(dst + vi * 16, v, tail);
        }
    }
    unsigned long long s1 = t + s0;

    for (int off = 32; off > 0; off >>= 1) {
        s0 += __shfl_down(s0, off, 64);
        s1 += __shfl_down(s1, off, 64);
    }
    __shared__ unsigned long long part[2][4];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[0][wave] = s0;
        part[1][wave] = s1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(&out[0], part[0][0] + part[0][1] + part[0][2] + part[0][3]);
        atomicAdd(&out[1], part[1][0] + part[1][1] + part[1][2] + part[1][3]);
    }
}

// Patch the master's segments that have a delta_off (layout rule above) with
// their bytes from the delta, scatter the nseg segments of the patched master
// to dst[k], and put csp_checksum_dev(master, arena_bytes) of the master as
// it is after the call into out[2].  Returns -1 with a message and launches
// nothing for every refusal of csp_unpack_checksum_dev (master in the place
// of its arena) and for: a misaligned delta, a null delta for a nonzero
// delta_bytes, a delta_off that breaks the delta layout rule, a delta_bytes
// that is not the rule's total, an overflow, or a delta range that overlaps
// the master or any destination range; ranges that merely touch are accepted.
// delta_bytes == 0 with every delta_off == UINT64_MAX is an unpack that
// leaves the master untouched.  Shares the unpack kernel's grid cap
// (csp_unpack_checksum_grid_cap).  Runs on copy_stream(), so it is ordered
// after the copies csp_h2d_stream_fd issued, and synchronises that stream
// before returning; buffers in use on another stream must be complete first.
// kernel_ms (optional): the kernel alone, from events around the launch.
extern "C" int csp_patch_unpack_checksum_dev(void* master, size_t arena_bytes,
                                             const void* delta, size_t delta_bytes,
                                             void* const* dst, const uint64_t* src_off,
                                             const uint64_t* nbytes,
                                             const uint64_t* delta_off, size_t nseg,
                                             uint64_t out[2], double* kernel_ms) {
    static const char* const fn = "csp_patch_unpack_checksum_dev";
    out[0] = out[1] = 0;
    if (kernel_ms) *kernel_ms = 0.0;
    const uintptr_t a = reinterpret_cast<uintptr_t>(master);
    const uintptr_t p = reinterpret_cast<uintptr_t>(delta);
    if (a % 16 != 0) {
        snprintf(g_err, sizeof(g_err), "%s: master pointer %p is not 16-byte aligned", fn,
                 master);
        return -1;
    }
    if (p % 16 != 0) {
        snprintf(g_err, sizeof(g_err), "%s: delta pointer %p is not 16-byte aligned", fn,
                 delta);
        return -1;
    }
    if (nseg >= (size_t(1) << 31)) {
        snprintf(g_err, sizeof(g_err), "%s: %zu segments are too many", fn, nseg);
        return -1;
    }
    if (a + arena_bytes < a) {
        snprintf(g_err, sizeof(g_err), "%s: %zu bytes at master %p overflow", fn, arena_bytes,
                 master);
        return -1;
    }
    if (p + delta_bytes < p) {
        snprintf(g_err, sizeof(g_err), "%s: %zu bytes at delta %p overflow", fn, delta_bytes,
                 delta);
        return -1;
    }
    std::vector<PatchSeg> table;
    table.reserve(nseg);
    uint64_t expect = 0, delta_expect = 0, tiles = 0;
    for (size_t k = 0; k < nseg; ++k) {
        if (src_off[k] != expect) {
            snprintf(g_err, sizeof(g_err),
                     "%s: src_off[%zu] is %llu, the layout rule gives %llu", fn, k,
                     (unsigned long long)src_off[k], (unsigned long long)expect);
            return -1;
        }
        const uint64_t rounded = (nbytes[k] + 15) & ~uint64_t(15);
        if (rounded < nbytes[k] || expect + rounded < expect) {
            snprintf(g_err, sizeof(g_err), "%s: segment %zu overflows", fn, k);
            return -1;
        }
        expect += rounded;
        const bool patched = delta_off[k] != UINT64_MAX;
        if (patched) {
            if (delta_off[k] != delta_expect) {
                snprintf(g_err, sizeof(g_err),
                         "%s: delta_off[%zu] is %llu, the delta layout rule gives %llu", fn, k,
                         (unsigned long long)delta_off[k], (unsigned long long)delta_expect);
                return -1;
            }
            delta_expect += rounded;  // <= expect: cannot overflow
        }
        const uintptr_t d = reinterpret_cast<uintptr_t>(dst[k]);
        if (d % 16 != 0) {
            snprintf(g_err, sizeof(g_err), "%s: dst[%zu] %p is not 16-byte aligned", fn, k,
                     dst[k]);
            return -1;
        }
        if (nbytes[k] == 0) continue;  // owns no tile
        if (d == 0) {
            snprintf(g_err, sizeof(g_err), "%s: segment %zu has %llu bytes and a null dst", fn,
                     k, (unsigned long long)nbytes[k]);
            return -1;
        }
        if (d + nbytes[k] < d) {
            snprintf(g_err, sizeof(g_err), "%s: dst[%zu] %p with %llu bytes overflows", fn, k,
                     dst[k], (unsigned long long)nbytes[k]);
            return -1;
        }
        table.push_back({static_cast<unsigned char*>(dst[k]),
                         patched ? static_cast<const unsigned char*>(delta) + delta_off[k]
                                 : nullptr,
                         src_off[k], nbytes[k], tiles});
        tiles += (rounded + kPackTileBytes - 1) / kPackTileBytes;
    }
    if (expect != (uint64_t)arena_bytes) {
        snprintf(g_err, sizeof(g_err), "%s: arena_bytes is %zu, the segments need %llu", fn,
                 arena_bytes, (unsigned long long)expect);
        return -1;
    }
    if (delta_expect != (uint64_t)delta_bytes) {
        snprintf(g_err, sizeof(g_err),
                 "%s: delta_bytes is %zu, the patched segments need %llu", fn, delta_bytes,
                 (unsigned long long)delta_expect);
        return -1;
    }
    if (arena_bytes == 0) return 0;
    if (master == nullptr) {
        snprintf(g_err, sizeof(g_err), "%s: null master for %zu bytes", fn, arena_bytes);
        return -1;
    }
    if (delta == nullptr && delta_bytes != 0) {
        snprintf(g_err, sizeof(g_err), "%s: null delta for %zu bytes", fn, delta_bytes);
        return -1;
    }
    if (delta_bytes != 0 && p < a + arena_bytes && a < p + delta_bytes) {
        snprintf(g_err, sizeof(g_err),
                 "%s: %zu bytes at delta %p overlap the master at %p", fn, delta_bytes, delta,
                 master);
        return -1;
    }
    for (size_t k = 0; k < table.size(); ++k) {
        const uintptr_t d = reinterpret_cast<uintptr_t>(table[k].dst);
        if (d < a + arena_bytes && a < d + table[k].nbytes) {
            snprintf(g_err, sizeof(g_err),
                     "%s: %llu bytes at dst %p overlap the master at %p", fn,
                     (unsigned long long)table[k].nbytes, (void*)table[k].dst, master);
            return -1;
        }
        if (delta_bytes != 0 && d < p + delta_bytes && p < d + table[k].nbytes) {
            snprintf(g_err, sizeof(g_err),
                     "%s: %llu bytes at dst %p overlap the delta at %p", fn,
                     (unsigned long long)table[k].nbytes, (void*)table[k].dst, delta);
            return -1;
        }
    }

    // one accumulator pair and one grow-only table per process, one call at
    // a time
    std::lock_guard<std::mutex> lock(g_checksum_mu);
    static unsigned long long* acc = nullptr;
    static PatchSeg* dev_table = nullptr;
    static size_t dev_cap = 0;  // entries
    static int dev_device = -1;
    int device = 0;
    HIP_TRY(hipGetDevice(&device));
    if (dev_device != device) {
        if (acc) (void)hipFree(acc);
        if (dev_table) (void)hipFree(dev_table);
        acc = nullptr;
        dev_table = nullptr;
        dev_cap = 0;
        dev_device = device;
    }
    if (acc == nullptr) HIP_TRY(hipMalloc(&acc, 2 * sizeof(unsigned long long)));
    if (dev_table == nullptr || dev_cap < table.size()) {
        if (dev_table) (void)hipFree(dev_table);
        dev_table = nullptr;
        dev_cap = 0;
        size_t cap = 1024;
        while (cap < table.size()) cap *= 2;
        HIP_TRY(hipMalloc(&dev_table, cap * sizeof(PatchSeg)));
        dev_cap = cap;
    }
    hipStream_t s = copy_stream();
    hipEvent_t t0 = nullptr, t1 = nullptr;
    if (kernel_ms) {
        HIP_TRY(hipEventCreate(&t0));
        hipError_t e = hipEventCreate(&t1);
        if (e != hipSuccess) {
            (void)hipEventDestroy(t0);
            return set_err("hipEventCreate", e);
        }
    }
    auto done = [&](int rc) {
        if (t0) (void)hipEventDestroy(t0);
        if (t1) (void)hipEventDestroy(t1);
        return rc;
    };
#define PATCH_TRY(expr)                                            \
    do {                                                           \
        hipError_t _e = (expr);                                    \
        if (_e != hipSuccess) return done(set_err(#expr, _e));     \
    } while (0)
    // `table` outlives the copy: the stream is synchronised below
    PATCH_TRY(hipMemcpyAsync(dev_table, table.data(), table.size() * sizeof(PatchSeg),
                             hipMemcpyHostToDevice, s));
    PATCH_TRY(hipMemsetAsync(acc, 0, 2 * sizeof(unsigned long long), s));
    const size_t blocks = tiles < g_unpack_grid_cap ? (size_t)tiles : g_unpack_grid_cap;
    if (t0) PATCH_TRY(hipEventRecord(t0, s));
    hipLaunchKernelGGL(csp_patch_unpack_checksum_kernel, dim3((unsigned int)blocks), dim3(256),
                       0, s, dev_table, (unsigned int)table.size(), (size_t)tiles,
                       static_cast<unsigned char*>(master), acc);
    PATCH_TRY(hipGetLastError());
    if (t1) PATCH_TRY(hipEventRecord(t1, s));
    unsigned long long host[2] = {0, 0};
    PATCH_TRY(hipMemcpyAsync(host, acc, sizeof(host), hipMemcpyDeviceToHost, s));
    PATCH_TRY(hipStreamSynchronize(s));
    if (kernel_ms) {
        float ms = 0.f;
        PATCH_TRY(hipEventElapsedTime(&ms, t0, t1));
        *kernel_ms = ms;
    }
#undef PATCH_TRY
    out[0] = host[0];
    out[1] = host[1];
    return done(0);
}

// ---------------------------------------------------------------------------
// Argument rebasing: a new master built from a held arena plus a delta
// ---------------------------------------------------------------------------
//
// The patch above consumes its base and needs the same layout.  A rebase
// builds a NEW arena of any layout and leaves the base alone: every segment
// of the new arena comes either from the base, at whatever 16-byte aligned
// offset it has there, or from a small delta arena, and the one pass that
// scatters and verifies the new arena also writes it out as a new master.
//
// Layout: out_off, nbytes, dst and arena_bytes follow the unpack layout rule
// for the NEW arena.  Exactly one of base_off[k] and delta_off[k] differs
// from UINT64_MAX.  The delta-sourced segments, in segment order, obey the
// pack layout inside the delta; base offsets are free: any order, shared by
// several new segments, base segments left out.
//
//   - the unpack and patch kernels' decomposition, unchanged: tiles of
//     kPackTileBytes of one segment, the host-built tile prefix, a binary
//     search per tile that depends on the tile index only, per-lane u64 s0/t
//     accumulators carried across a block's tiles, wave shuffles, LDS, one
//     atomicAdd pair per block, 256-thread blocks, the unpack kernel's grid
//     cap;
//   - the table entry holds an absolute source pointer and a from_delta flag:
//     delta loads are nontemporal (read once), base loads are plain (the base
//     is re-read by later hits); the choice is per tile and wave-uniform;
//   - every vector a segment owns is loaded once, stored whole to
//     out_arena + out_off with a plain aligned 16-byte store (the new master
//     is re-read by the next hit; the last vector's padding goes in as the
//     source has it), stored to dst by the unpack rules and summed with the
//     word index global to the new arena;
//   - out_arena == nullptr is a transient rebase: the same scatter and sum,
//     no new master written; the branch is on a kernel argument, so uniform;
//   - base and delta are never written, and the host refuses an out_arena
//     that overlaps either or any dst, so no lane reads what another writes.
struct RebaseSeg {
    unsigned char* dst;
    const unsigned char* src;  // absolute: into the base or into the delta
    unsigned long long out_off;
    unsigned long long nbytes;
    unsigned long long tile_begin;  // tiles owned by the segments before this one
    unsigned long long from_delta;  // nonzero: src is in the delta
};

__global__ __launch_bounds__(256) void csp_rebase_unpack_checksum_kernel(
    const RebaseSeg* __restrict__ segs, unsigned int nseg, size_t total_tiles,
    unsigned char* out_arena, unsigned long long* __restrict__ out) {
    unsigned long long s0 = 0, t = 0;
    const bool keep = out_arena != nullptr;  // kernel argument: uniform
    for (size_t tile = blockIdx.x; tile < total_tiles; tile += gridDim.x) {
        // last segment whose first tile is <= tile (tile_begin is strictly
        // increasing: the host leaves zero-byte segments out of the table)
        unsigned int lo = 0, hi = nseg;
        while (hi - lo > 1) {
            const unsigned int mid = (lo + hi) / 2;
            if (segs[mid].tile_begin <= tile) lo = mid; else hi = mid;
        }
        const RebaseSeg s = segs[lo];
        const CSP_GLOBAL u32x4* src = reinterpret_cast<const CSP_GLOBAL u32x4*>(
            (const CSP_GLOBAL unsigned char*)s.src);
        CSP_GLOBAL u32x4* mst = reinterpret_cast<CSP_GLOBAL u32x4*>(
            (CSP_GLOBAL unsigned char*)(out_arena + s.out_off));
        const bool from_delta = s.from_delta != 0;  // per tile: wave-uniform
        const unpack_dst_t dst = (unpack_dst_t)s.dst;
        const size_t nfull = s.nbytes / 16;  // vectors wholly inside the segment
        const unsigned int tail = (unsigned int)(s.nbytes % 16);
        const size_t nvec = nfull + (tail ? 1 : 0);  // vectors the segment owns
        const size_t v0 = (tile - s.tile_begin) * kPackTileVecs + threadIdx.x;
        // new-arena-global index of the segment's first word, modulo 2^32
        // like csp_checksum_kernel's (unsigned int)(i * 4)
        const unsigned int word_base = (unsigned int)(s.out_off / 4);
        if ((tile - s.tile_begin + 1) * kPackTileVecs <= nfull) {
            // interior tile: every lane has four whole vectors
            u32x4 v[kPackUnroll];
            if (from_delta) {
#pragma unroll
                for (int u = 0; u < kPackUnroll; ++u)
                    v[u] = __builtin_nontemporal_load(&src[v0 + u * 256]);
            } else {
#pragma unroll
                for (int u = 0; u < kPackUnroll; ++u) v[u] = src[v0 + u * 256];
            }
            if (keep) {
#pragma unroll
                for (int u = 0; u < kPackUnroll; ++u) mst[v0 + u * 256] = v[u];
            }
#pragma unroll
            for (int u = 0; u < kPackUnroll; ++u) {
                const size_t vi = v0 + u * 256;
                __builtin_nontemporal_store(
                    v[u], reinterpret_cast<CSP_GLOBAL u32x4*>(dst + vi * 16));
                checksum_add(s0, t, v[u], word_base + (unsigned int)(vi * 4));
            }
            continue;
        }
#pragma unroll
        for (int u = 0; u < kPackUnroll; ++u) {
            const size_t vi = v0 + u * 256;
            if (vi >= nvec) continue;
            u32x4 v;  // padding included: all 16 bytes are base or delta
            if (from_delta)
                v = __builtin_nontemporal_load(&src[vi]);
            else
                v = src[vi];
            if (keep) mst[vi] = v;
            checksum_add(s0, t, v, word_base + (unsigned int)(vi * 4));
            if (vi < nfull)
                __builtin_nontemporal_store(
                    v, reinterpret_cast<CSP_GLOBAL u32x4*>(dst + vi * 16));
            else
                unpack_store_tail(dst + vi * 16, v, tail);
        }
    }
    unsigned long long s1 = t + s0;

    for (int off = 32; off > 0; off >>= 1) {
        s0 += __shfl_down(s0, off, 64);
        s1 += __shfl_down(s1, off, 64);
    }
    __shared__ unsigned long long part[2][4];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[0][wave] = s0;
        part[1][wave] = s1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(&out[0], part[0][0] + part[0][1] + part[0][2] + part[0][3]);
        atomicAdd(&out[1], part[1][0] + part[1][1] + part[1][2] + part[1][3]);
    }
}

// Build the new arena's nseg segments (layout rule above) from the base and
// the delta, scatter them to dst[k], write them to out_arena unless it is
// null, and put csp_checksum_dev's (s0, s1) of the new arena into out[2].
// Returns -1 with a message and launches nothing for every refusal of
// csp_unpack_checksum_dev on the new layout (out_off in the place of its
// src_off) and for: a misaligned base, delta or out_arena; a base_off that is
// not a multiple of 16 or with base_off + round_up(nbytes, 16) > base_bytes; a
// segment with both sources or with neither; a delta_off that breaks the
// delta layout rule or a delta_bytes that is not its total; a null base or
// delta where bytes are to come from it; an overflow; out_arena overlapping
// the base, the delta or any dst; any dst overlapping the base or the delta.
// Ranges that merely touch are accepted, and so are base and delta ranges
// that overlap each other: both are only read.  Overlap between destinations
// is the caller's responsibility, as in the unpack.  Shares the unpack
// kernel's grid cap (csp_unpack_checksum_grid_cap).  Runs on copy_stream()
// and synchronises it before returning.  kernel_ms (optional): the kernel
// alone, from events around the launch.
extern "C" int csp_rebase_unpack_checksum_dev(const void* base, size_t base_bytes,
                                              const void* delta, size_t delta_bytes,
                                              void* out_arena, size_t arena_bytes,
                                              void* const* dst, const uint64_t* out_off,
                                              const uint64_t* nbytes,
                                              const uint64_t* base_off,
                                              const uint64_t* delta_off, size_t nseg,
                                              uint64_t out[2], double* kernel_ms) {
    static const char* const fn = "csp_rebase_unpack_checksum_dev";
    out[0] = out[1] = 0;
    if (kernel_ms) *kernel_ms = 0.0;
    const uintptr_t b = reinterpret_cast<uintptr_t>(base);
    const uintptr_t p = reinterpret_cast<uintptr_t>(delta);
    const uintptr_t a = reinterpret_cast<uintptr_t>(out_arena);
    if (b % 16 != 0) {
        snprintf(g_err, sizeof(g_err), "%s: base pointer %p is not 16-byte aligned", fn, base);
        return -1;
    }
    if (p % 16 != 0) {
        snprintf(g_err, sizeof(g_err), "%s: delta pointer %p is not 16-byte aligned", fn,
                 delta);
        return -1;
    }
    if (a % 16 != 0) {
        snprintf(g_err, sizeof(g_err), "%s: out_arena pointer %p is not 16-byte aligned", fn,
                 out_arena);
        return -1;
    }
    if (nseg >= (size_t(1) << 31)) {
        snprintf(g_err, sizeof(g_err), "%s: %zu segments are too many", fn, nseg);
        return -1;
    }
    if (b + base_bytes < b) {
        snprintf(g_err, sizeof(g_err), "%s: %zu bytes at base %p overflow", fn, base_bytes,
                 base);
        return -1;
    }
    if (p + delta_bytes < p) {
        snprintf(g_err, sizeof(g_err), "%s: %zu bytes at delta %p overflow", fn, delta_bytes,
                 delta);
        return -1;
    }
    if (a + arena_bytes < a) {
        snprintf(g_err, sizeof(g_err), "%s: %zu bytes at out_arena %p overflow", fn,
                 arena_bytes, out_arena);
        return -1;
    }
    std::vector<RebaseSeg> table;
    table.reserve(nseg);
    uint64_t expect = 0, delta_expect = 0, tiles = 0;
    bool base_used = false;
    for (size_t k = 0; k < nseg; ++k) {
        if (out_off[k] != expect) {
            snprintf(g_err, sizeof(g_err),
                     "%s: out_off[%zu] is %llu, the layout rule gives %llu", fn, k,
                     (unsigned long long)out_off[k], (unsigned long long)expect);
            return -1;
        }
        const uint64_t rounded = (nbytes[k] + 15) & ~uint64_t(15);
        if (rounded < nbytes[k] || expect + rounded < expect) {
            snprintf(g_err, sizeof(g_err), "%s: segment %zu overflows", fn, k);
            return -1;
        }
        expect += rounded;
        const bool from_base = base_off[k] != UINT64_MAX;
        const bool from_delta = delta_off[k] != UINT64_MAX;
        if (from_base == from_delta) {
            snprintf(g_err, sizeof(g_err), "%s: segment %zu has %s", fn, k,
                     from_base ? "both a base_off and a delta_off"
                               : "neither a base_off nor a delta_off");
            return -1;
        }
        if (from_delta) {
            if (delta_off[k] != delta_expect) {
                snprintf(g_err, sizeof(g_err),
                         "%s: delta_off[%zu] is %llu, the delta layout rule gives %llu", fn, k,
                         (unsigned long long)delta_off[k], (unsigned long long)delta_expect);
                return -1;
            }
            delta_expect += rounded;  // <= expect: cannot overflow
        } else {
            if (base_off[k] % 16 != 0) {
                snprintf(g_err, sizeof(g_err),
                         "%s: base_off[%zu] is %llu, not a multiple of 16", fn, k,
                         (unsigned long long)base_off[k]);
                return -1;
            }
            if (base_off[k] > (uint64_t)base_bytes ||
                rounded > (uint64_t)base_bytes - base_off[k]) {
                snprintf(g_err, sizeof(g_err),
                         "%s: base_off[%zu] %llu with %llu rounded bytes exceeds the base's %zu",
                         fn, k, (unsigned long long)base_off[k], (unsigned long long)rounded,
                         base_bytes);
                return -1;
            }
        }
        const uintptr_t d = reinterpret_cast<uintptr_t>(dst[k]);
        if (d % 16 != 0) {
            snprintf(g_err, sizeof(g_err), "%s: dst[%zu] %p is not 16-byte aligned", fn, k,
                     dst[k]);
            return -1;
        }
        if (nbytes[k] == 0) continue;  // owns no tile
        if (d == 0) {
            snprintf(g_err, sizeof(g_err), "%s: segment %zu has %llu bytes and a null dst", fn,
                     k, (unsigned long long)nbytes[k]);
            return -1;
        }
        if (d + nbytes[k] < d) {
            snprintf(g_err, sizeof(g_err), "%s: dst[%zu] %p with %llu bytes overflows", fn, k,
                     dst[k], (unsigned long long)nbytes[k]);
            return -1;
        }
        if (from_base) base_used = true;
        table.push_back({static_cast<unsigned char*>(dst[k]),
                         from_delta ? static_cast<const unsigned char*>(delta) + delta_off[k]
                                    : static_cast<const unsigned char*>(base) + base_off[k],
                         out_off[k], nbytes[k], tiles, from_delta ? 1ull : 0ull});
        tiles += (rounded + kPackTileBytes - 1) / kPackTileBytes;
    }
    if (expect != (uint64_t)arena_bytes) {
        snprintf(g_err, sizeof(g_err), "%s: arena_bytes is %zu, the segments need %llu", fn,
                 arena_bytes, (unsigned long long)expect);
        return -1;
    }
    if (delta_expect != (uint64_t)delta_bytes) {
        snprintf(g_err, sizeof(g_err),
                 "%s: delta_bytes is %zu, the delta-sourced segments need %llu", fn,
                 delta_bytes, (unsigned long long)delta_expect);
        return -1;
    }
    if (arena_bytes == 0) return 0;
    if (base == nullptr && base_used) {
        snprintf(g_err, sizeof(g_err), "%s: null base for base-sourced segments", fn);
        return -1;
    }
    if (delta == nullptr && delta_bytes != 0) {
        snprintf(g_err, sizeof(g_err), "%s: null delta for %zu bytes", fn, delta_bytes);
        return -1;
    }
    if (out_arena != nullptr) {
        if (base_bytes != 0 && a < b + base_bytes && b < a + arena_bytes) {
            snprintf(g_err, sizeof(g_err),
                     "%s: %zu bytes at out_arena %p overlap the base at %p", fn, arena_bytes,
                     out_arena, base);
            return -1;
        }
        if (delta_bytes != 0 && a < p + delta_bytes && p < a + arena_bytes) {
            snprintf(g_err, sizeof(g_err),
                     "%s: %zu bytes at out_arena %p overlap the delta at %p", fn, arena_bytes,
                     out_arena, delta);
            return -1;
        }
    }
    for (size_t k = 0; k < table.size(); ++k) {
        const uintptr_t d = reinterpret_cast<uintptr_t>(table[k].dst);
        if (out_arena != nullptr && d < a + arena_bytes && a < d + table[k].nbytes) {
            snprintf(g_err, sizeof(g_err),
                     "%s: %llu bytes at dst %p overlap the out_arena at %p", fn,
                     (unsigned long long)table[k].nbytes, (void*)table[k].dst, out_arena);
            return -1;
        }
        if (base_bytes != 0 && d < b + base_bytes && b < d + table[k].nbytes) {
            snprintf(g_err, sizeof(g_err),
                     "%s: %llu bytes at dst %p overlap the base at %p", fn,
                     (unsigned long long)table[k].nbytes, (void*)table[k].dst, base);
            return -1;
        }
        if (delta_bytes != 0 && d < p + delta_bytes && p < d + table[k].nbytes) {
            snprintf(g_err, sizeof(g_err),
                     "%s: %llu bytes at dst %p overlap the delta at %p", fn,
                     (unsigned long long)table[k].nbytes, (void*)table[k].dst, delta);
            return -1;
        }
    }

    // one accumulator pair and one grow-only table per process, one call at
    // a time
    std::lock_guard<std::mutex> lock(g_checksum_mu);
    static unsigned long long* acc = nullptr;
    static RebaseSeg* dev_table = nullptr;
    static size_t dev_cap = 0;  // entries
    static int dev_device = -1;
    int device = 0;
    HIP_TRY(hipGetDevice(&device));
    if (dev_device != device) {
        if (acc) (void)hipFree(acc);
        if (dev_table) (void)hipFree(dev_table);
        acc = nullptr;
        dev_table = nullptr;
        dev_cap = 0;
        dev_device = device;
    }
    if (acc == nullptr) HIP_TRY(hipMalloc(&acc, 2 * sizeof(unsigned long long)));
    if (dev_table == nullptr || dev_cap < table.size()) {
        if (dev_table) (void)hipFree(dev_table);
        dev_table = nullptr;
        dev_cap = 0;
        size_t cap = 1024;
        while (cap < table.size()) cap *= 2;
        HIP_TRY(hipMalloc(&dev_table, cap * sizeof(RebaseSeg)));
        dev_cap = cap;
    }
    hipStream_t s = copy_stream();
    hipEvent_t t0 = nullptr, t1 = nullptr;
    if (kernel_ms) {
        HIP_TRY(hipEventCreate(&t0));
        hipError_t e = hipEventCreate(&t1);
        if (e != hipSuccess) {
            (void)hipEventDestroy(t0);
            return set_err("hipEventCreate", e);
        }
    }
    auto done = [&](int rc) {
        if (t0) (void)hipEventDestroy(t0);
        if (t1) (void)hipEventDestroy(t1);
        return rc;
    };
#define REBASE_TRY(expr)                                           \
    do {                                                           \
        hipError_t _e = (expr);                                    \
        if (_e != hipSuccess) return done(set_err(#expr, _e));     \
    } while (0)
    // `table` outlives the copy: the stream is synchronised below
    REBASE_TRY(hipMemcpyAsync(dev_table, table.data(), table.size() * sizeof(RebaseSeg),
                              hipMemcpyHostToDevice, s));
    REBASE_TRY(hipMemsetAsync(acc, 0, 2 * sizeof(unsigned long long), s));
    const size_t blocks = tiles < g_unpack_grid_cap ? (size_t)tiles : g_unpack_grid_cap;
    if (t0) REBASE_TRY(hipEventRecord(t0, s));
    hipLaunchKernelGGL(csp_rebase_unpack_checksum_kernel, dim3((unsigned int)blocks),
                       dim3(256), 0, s, dev_table, (unsigned int)table.size(), (size_t)tiles,
                       static_cast<unsigned char*>(out_arena), acc);
    REBASE_TRY(hipGetLastError());
    if (t1) REBASE_TRY(hipEventRecord(t1, s));
    unsigned long long host[2] = {0, 0};
    REBASE_TRY(hipMemcpyAsync(host, acc, sizeof(host), hipMemcpyDeviceToHost, s));
    REBASE_TRY(hipStreamSynchronize(s));
    if (kernel_ms) {
        float ms = 0.f;
        REBASE_TRY(hipEventElapsedTime(&ms, t0, t1));
        *kernel_ms = ms;
    }
#undef REBASE_TRY
    out[0] = host[0];
    out[1] = host[1];
    return done(0);
}

// On-box variant exploration for the HBM sweep (tools only; the probe
// uses g_sweep_variant).  Returns measured GB/s via *gbps.
extern "C" int csp_hbm_bench(int device, int variant, size_t bytes, int reps,
                             double* gbps) {
    HIP_TRY(hipSetDevice(device));
    size_t n4 = bytes / sizeof(float4);
    float4 *a = nullptr, *b = nullptr;
    HIP_TRY(hipMalloc(&a, bytes));
    HIP_TRY(hipMalloc(&b, bytes));
    HIP_TRY(hipMemsetAsync(a, 1, bytes));
    float warm_ms = 0.f, ms = 0.f;
    int rc = run_hbm_sweep(a, b, n4, 2, &warm_ms, variant);
    if (rc == 0) rc = run_hbm_sweep(a, b, n4, reps, &ms, variant);
    (void)hipFree(a);
    (void)hipFree(b);
    if (rc != 0) return rc;
    *gbps = (2.0 * (double)bytes * reps / 1.0e9) / ((double)ms / 1000.0);
    return 0;
}

// Extended exploration: grid size + copy direction knobs.
extern "C" int csp_hbm_bench2(int device, int variant, size_t bytes, int reps,
                              int blocks, int pingpong, double* gbps) {
    HIP_TRY(hipSetDevice(device));
    size_t n4 = bytes / sizeof(float4);
    float4 *a = nullptr, *b = nullptr;
    HIP_TRY(hipMalloc(&a, bytes));
    HIP_TRY(hipMalloc(&b, bytes));
    HIP_TRY(hipMemsetAsync(a, 1, bytes));
    float warm_ms = 0.f, ms = 0.f;
    int rc = run_hbm_sweep(a, b, n4, 2, &warm_ms, variant, blocks, pingpong != 0);
    if (rc == 0)
        rc = run_hbm_sweep(a, b, n4, reps, &ms, variant, blocks, pingpong != 0);
    (void)hipFree(a);
    (void)hipFree(b);
    if (rc != 0) return rc;
    *gbps = (2.0 * (double)bytes * reps / 1.0e9) / ((double)ms / 1000.0);
    return 0;
}

// MFMA spin exploration: blocks knob (TF/s out).
extern "C" int csp_mfma_bench(int device, int iters, int blocks, double* tflops) {
    HIP_TRY(hipSetDevice(device));
    float ms = 0.f;
    int rc = run_mfma_spin(iters / 4, blocks, &ms);  // warm clocks
    if (rc == 0) rc = run_mfma_spin(iters, blocks, &ms);
    if (rc != 0) return rc;
    double waves = (double)blocks * 4.0;
    *tflops = waves * (double)iters * kFlopPerMfma / ((double)ms / 1000.0) / 1.0e12;
    return 0;
}

// ---------------------------------------------------------------------------
// MFMA numerics check: one v_mfma_f32_32x32x16_bf16 with self-described
// operand layouts.  Each lane scatters the exact operand values it feeds
// the instruction into global A (32x16) and B (16x32), and its
// accumulator fragment into D (32x32) using the C/D mapping
// (col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)).  The host
// test then asserts D == A @ B against a PyTorch reference — validating
// the assumed A/B lane mapping AND the instruction together.  `layout`
// selects the A/B k-mapping candidate:
//   0: k = (lane>>5)*8 + j           (contiguous 8)
//   1: k = (lane>>5)*4 + (j&3) + (j>>2)*8   (two 4-element halves)
__global__ __launch_bounds__(64) void csp_mfma_check_kernel(
    float* __restrict__ D, float* __restrict__ A, float* __restrict__ B,
    int layout) {
    const int l = threadIdx.x;
    bf16x8 a, b;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = (layout == 0) ? ((l >> 5) * 8 + j)
                                    : ((l >> 5) * 4 + (j & 3) + (j >> 2) * 8);
        const int i = l & 31;  // A row
        const float av = (float)(((i * 3 + k) % 7) - 3);  // integer-valued
        a[j] = (__bf16)av;
        A[i * 16 + k] = av;
        const int col = l & 31;  // B column
        const float bv = (float)(((k * 5 + col) % 5) - 2);
        b[j] = (__bf16)bv;
        B[k * 32 + col] = bv;
    }
    f32x16 acc = {};
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
        D[row * 32 + (l & 31)] = acc[r];
    }
}

extern "C" int csp_mfma_check(int device, int layout, float* d_out,
                              float* a_out, float* b_out) {
    HIP_TRY(hipSetDevice(device));
    float *D = nullptr, *A = nullptr, *B = nullptr;
    HIP_TRY(hipMalloc(&D, 32 * 32 * sizeof(float)));
    HIP_TRY(hipMalloc(&A, 32 * 16 * sizeof(float)));
    HIP_TRY(hipMalloc(&B, 16 * 32 * sizeof(float)));
    hipLaunchKernelGGL(csp_mfma_check_kernel, dim3(1), dim3(64), 0, 0, D, A, B,
                       layout);
    HIP_TRY(hipMemcpy(d_out, D, 32 * 32 * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(a_out, A, 32 * 16 * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(b_out, B, 16 * 32 * sizeof(float), hipMemcpyDeviceToHost));
    (void)hipFree(D);
    (void)hipFree(A);
    (void)hipFree(B);
    return 0;
}
