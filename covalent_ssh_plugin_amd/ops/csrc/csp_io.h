// Exact-length fd I/O shared by libcsp_io.so (csp_io.cpp, host only) and
// libcsp_gpu.so (csp_gpu.hip, the streaming D2H sender).  Header-only so
// the GPU library does not have to link the host library; no HIP, no ROCm.
//
// Also the host half of the argument checksum (checksum() below); the GPU
// half is csp_checksum_kernel in csp_gpu.hip and must agree bit for bit.
//
// Return codes (the C ABI in csp_io.cpp passes them through):
//   CSP_IO_OK       all n bytes moved
//   CSP_IO_EOF      read side only: the peer closed before n bytes arrived
//   CSP_IO_TIMEOUT  read side only: no byte became available for timeout_ms
//   -errno          any other failure (a closed reader gives -EPIPE)

#pragma once

#include <cerrno>
#include <csignal>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <ctime>

#include <poll.h>
#include <pthread.h>
#include <unistd.h>

#define CSP_IO_OK 0
#define CSP_IO_EOF 1
#define CSP_IO_TIMEOUT 2

namespace csp_io_detail {

// One syscall moves at most this much: keeps a single read()/write() well
// inside ssize_t and lets a signal be noticed between pieces.
static const size_t kMaxPiece = size_t(1) << 30;

// poll() one fd for `events`.  timeout_ms < 0 waits without limit.
// Returns 1 when ready, 0 on timeout, -errno on failure.
static inline int wait_fd(int fd, short events, int timeout_ms) {
    for (;;) {
        struct pollfd p;
        p.fd = fd;
        p.events = events;
        p.revents = 0;
        int rc = poll(&p, 1, timeout_ms);
        if (rc > 0) return 1;  // readable/writable, or HUP/ERR: let the I/O call report it
        if (rc == 0) return 0;
        if (errno != EINTR) return -errno;
    }
}

// Read exactly n bytes into dst.  timeout_ms bounds every wait for the
// NEXT byte (an idle limit, not a limit on the whole transfer); < 0 means
// no limit.  Never asks the kernel for more than the bytes still missing,
// so nothing past the n-th byte is consumed.  *done (optional) receives
// the number of bytes placed in dst, whatever the outcome.
static inline int read_full(int fd, void* dst, size_t n, int timeout_ms,
                            size_t* done) {
    char* p = static_cast<char*>(dst);
    size_t got = 0;
    int rc = CSP_IO_OK;
    while (got < n) {
        if (timeout_ms >= 0) {
            // poll first, blocking fds included: a blocking read() on a
            // silent peer would otherwise never come back
            int w = wait_fd(fd, POLLIN, timeout_ms);
            if (w == 0) { rc = CSP_IO_TIMEOUT; break; }
            if (w < 0) { rc = w; break; }
        }
        size_t want = n - got;
        if (want > kMaxPiece) want = kMaxPiece;
        ssize_t r = read(fd, p + got, want);
        if (r > 0) { got += size_t(r); continue; }
        if (r == 0) { rc = CSP_IO_EOF; break; }
        if (errno == EINTR) continue;
        if (errno == EAGAIN || errno == EWOULDBLOCK) {
            if (timeout_ms >= 0) continue;  // the poll above does the waiting
            int w = wait_fd(fd, POLLIN, -1);
            if (w < 0) { rc = w; break; }
            continue;
        }
        rc = -errno;
        break;
    }
    if (done) *done = got;
    return rc;
}

// Write exactly n bytes from src.  SIGPIPE is held back for the calling
// thread while it writes, so a closed reader comes back as -EPIPE even in
// a process that left the signal at its default action.
static inline int write_full(int fd, const void* src, size_t n, size_t* done) {
    const char* p = static_cast<const char*>(src);
    size_t put = 0;
    int rc = CSP_IO_OK;

    sigset_t pipe_set, old_set, pending;
    sigemptyset(&pipe_set);
    sigaddset(&pipe_set, SIGPIPE);
    bool was_pending = false;
    bool masked = pthread_sigmask(SIG_BLOCK, &pipe_set, &old_set) == 0;
    if (masked && sigpending(&pending) == 0)
        was_pending = sigismember(&pending, SIGPIPE) == 1;

    while (put < n) {
        size_t want = n - put;
        if (want > kMaxPiece) want = kMaxPiece;
        ssize_t w = write(fd, p + put, want);
        if (w >= 0) { put += size_t(w); continue; }
        if (errno == EINTR) continue;
        if (errno == EAGAIN || errno == EWOULDBLOCK) {
            int r = wait_fd(fd, POLLOUT, -1);
            if (r < 0) { rc = r; break; }
            continue;
        }
        rc = -errno;
        break;
    }

    if (masked) {
        if (rc == -EPIPE && !was_pending) {
            // take our own SIGPIPE off the thread before unmasking
            struct timespec zero = {0, 0};
            while (sigtimedwait(&pipe_set, nullptr, &zero) < 0 && errno == EINTR) {
            }
        }
        pthread_sigmask(SIG_SETMASK, &old_set, nullptr);
    }
    if (done) *done = put;
    return rc;
}

// Checksum of n payload bytes, identical on host and GPU.  The bytes are
// taken as little-endian u32 words w_0 .. w_{m-1}, m = ceil(n/4), the last
// word zero-padded; both sums wrap modulo 2^64:
//   out[0] = sum w_i
//   out[1] = sum w_i * ((i mod 2^32) + 1)
// Integer addition is associative, so any reduction order gives the same
// two numbers.  Any pointer alignment, any n; n == 0 gives (0, 0).
//
// The loop adds w_i * (i mod 2^32), a u32 x u32 -> u64 product that the
// compiler can vectorise, and the "+ 1" term is out[0] added once at the
// end.
static inline void checksum(const void* src, size_t n, uint64_t out[2]) {
    const unsigned char* p = static_cast<const unsigned char*>(src);
    const size_t full = n / 4;
    uint64_t s0 = 0, s1 = 0;
    uint32_t idx = 0;  // i mod 2^32, kept 32 bits wide so the product stays u32 x u32
    for (size_t i = 0; i < full; ++i, ++idx) {
        uint32_t w;
        memcpy(&w, p + 4 * i, 4);  // unaligned-safe; little-endian hosts only
        s0 += w;
        s1 += uint64_t(w) * idx;
    }
    if (n & 3) {
        uint32_t w = 0;
        memcpy(&w, p + 4 * full, n & 3);
        s0 += w;
        s1 += uint64_t(w) * uint32_t(full);
    }
    out[0] = s0;
    out[1] = s1 + s0;
}

// The host half of lossless narrowing (narrow_tensor_args): what
// csp_narrow_checksum_kernel in csp_gpu.hip does to a result on the GPU, done
// to an argument where it leaves.  Exactness is decided on the bits by the
// rules of the block comment above that kernel, the CPU's float conversion
// takes no part, and `bad` has that kernel's meaning: for floats the bits
// that had to be zero (bit 63: wrong class of value), for integers the OR of
// x ^ (x >> sign) and in bit 63 the OR of the signs.  csp_widen_checksum_kernel
// gives back exactly what a clean `bad` let through.
static const uint64_t kNarrowFlag = uint64_t(1) << 63;
enum { kKindF32 = 0, kKindF64 = 1, kKindI32 = 2, kKindI64 = 3, kKindBF16 = 4, kKindI16 = 5,
       kKindU8 = 6 };

static inline uint16_t narrow_f32(uint32_t x, uint64_t& bad) {
    bad |= x & 0xFFFFu;
    return uint16_t(x >> 16);
}

static inline uint32_t narrow_f64(uint64_t x, uint64_t& bad) {
    const uint32_t lo = uint32_t(x), hi = uint32_t(x >> 32);
    const uint32_t e = (hi >> 20) & 0x7FFu;
    const uint32_t mhi = hi & 0xFFFFFu;  // the top 20 mantissa bits
    const bool zero = (e | mhi | lo) == 0;
    const bool normal = e - 897u <= 1150u - 897u;  // unbiased -126..127
    const bool inf_or_quiet = e == 0x7FFu && ((mhi | lo) == 0 || (mhi & 0x80000u) != 0);
    bad |= (lo & 0x1FFFFFFFu) | ((zero || normal || inf_or_quiet) ? uint64_t(0) : kNarrowFlag);
    const uint32_t e32 = zero ? 0u : (e == 0x7FFu ? 0xFFu : ((e - 896u) & 0xFFu));
    return (hi & 0x80000000u) | (e32 << 23) | (mhi << 3) | (lo >> 29);
}

template <typename D> static inline D narrow_i64(uint64_t x, uint64_t& bad) {
    const int64_t s = int64_t(x);
    bad |= uint64_t(s ^ (s >> 63)) | (x & kNarrowFlag);
    return D(x);  // the low bytes
}

template <typename D> static inline D narrow_i32(uint32_t x, uint64_t& bad) {
    const int32_t s = int32_t(x);
    bad |= uint32_t(s ^ (s >> 31)) | (uint64_t(x & 0x80000000u) << 32);
    return D(x);
}

// numel elements of S at src through f; the narrow ones to dst when it is set
template <typename S, typename D, D (*F)(S, uint64_t&)>
static inline void narrow_loop(const void* src, size_t numel, void* dst, uint64_t* bad) {
    const unsigned char* p = static_cast<const unsigned char*>(src);
    unsigned char* q = static_cast<unsigned char*>(dst);
    uint64_t b = 0;
    for (size_t i = 0; i < numel; ++i) {
        S x;
        memcpy(&x, p + i * sizeof(S), sizeof(S));  // unaligned-safe; little-endian hosts only
        const D y = F(x, b);
        if (q) memcpy(q + i * sizeof(D), &y, sizeof(D));
    }
    *bad |= b;
}

// One pass over numel elements of src_kind: ORs into *bad what speaks against
// narrowing them exactly and, when dst is set, writes them narrowed to
// dst_kind (numel * its element size bytes), whatever the verdict.  Kinds and
// pairs are csp_narrow_checksum_dev's.  Returns 0, or -1 for a pair that is
// not served or a null bad.
static inline int narrow(const void* src, size_t numel, int src_kind, int dst_kind, void* dst,
                         uint64_t* bad) {
    if (bad == nullptr) return -1;
    switch (src_kind * 8 + dst_kind) {
    case kKindF32 * 8 + kKindBF16:
        narrow_loop<uint32_t, uint16_t, narrow_f32>(src, numel, dst, bad);
        return 0;
    case kKindF64 * 8 + kKindF32:
        narrow_loop<uint64_t, uint32_t, narrow_f64>(src, numel, dst, bad);
        return 0;
    case kKindI64 * 8 + kKindI32:
        narrow_loop<uint64_t, uint32_t, narrow_i64<uint32_t>>(src, numel, dst, bad);
        return 0;
    case kKindI64 * 8 + kKindI16:
        narrow_loop<uint64_t, uint16_t, narrow_i64<uint16_t>>(src, numel, dst, bad);
        return 0;
    case kKindI64 * 8 + kKindU8:
        narrow_loop<uint64_t, uint8_t, narrow_i64<uint8_t>>(src, numel, dst, bad);
        return 0;
    case kKindI32 * 8 + kKindI16:
        narrow_loop<uint32_t, uint16_t, narrow_i32<uint16_t>>(src, numel, dst, bad);
        return 0;
    case kKindI32 * 8 + kKindU8:
        narrow_loop<uint32_t, uint8_t, narrow_i32<uint8_t>>(src, numel, dst, bad);
        return 0;
    }
    return -1;
}

// The host half of the "bits" wire format (bool tensors under
// narrow_tensor_args), what csp_bool_pack_checksum_kernel in csp_gpu.hip does
// to a result: element i is bit i % 8 of byte i / 8, as numpy.packbits with
// bitorder="little".  A bool tensor is exact iff every storage byte is 0 or 1;
// `bad` gets the OR of byte & 0xFE.  A caller that cuts a tensor into pieces
// starts every piece on a multiple of 8 elements, so that no two pieces share
// an output byte.  With dst set, (numel + 7) / 8 bytes are written, the pad
// bits of the last one zero, whatever the verdict.  Returns 0, or -1 for a
// null bad.
static inline int bool_pack(const void* src, size_t numel, void* dst, uint64_t* bad) {
    if (bad == nullptr) return -1;
    const unsigned char* p = static_cast<const unsigned char*>(src);
    unsigned char* q = static_cast<unsigned char*>(dst);
    uint64_t b = 0;
    size_t i = 0;
    for (; i + 8 <= numel; i += 8) {
        uint64_t w;
        memcpy(&w, p + i, 8);  // little-endian hosts only
        b |= w & 0xFEFEFEFEFEFEFEFEull;
        // bit 8 * j of w to bit 56 + j: the products' bits do not collide
        const uint64_t bits = (w & 0x0101010101010101ull) * 0x0102040810204080ull;
        if (q) q[i / 8] = (unsigned char)(bits >> 56);
    }
    if (i < numel) {
        unsigned char o = 0;
        for (size_t j = i; j < numel; ++j) {
            b |= p[j] & 0xFEu;
            o |= (unsigned char)((p[j] & 1u) << (j - i));
        }
        if (q) q[i / 8] = o;
    }
    b |= b >> 32;  // the eight byte lanes of the word loop folded into one
    b |= b >> 16;
    b |= b >> 8;
    *bad |= b & 0xFEu;
    return 0;
}

}  // namespace csp_io_detail
