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

}  // namespace csp_io_detail
