// Host-only native I/O for the dispatcher side of the worker channel
// (libcsp_io.so).  Plain C ABI for ctypes; no HIP, no ROCm: a dispatcher
// with only a CPU loads it.
//
//   csp_io_read_full   read exactly n bytes from an fd straight into the
//                      caller's buffer: one kernel-to-destination copy for
//                      a large tensor frame, off the event-loop thread
//                      (ctypes drops the GIL for the call)
//   csp_io_write_full  the same contract for writes
//   csp_io_alloc/free  anonymous mapping that asks for transparent huge
//                      pages, as the destination of a large frame
//   csp_io_checksum    the two-word argument checksum (definition in
//                      csp_io.h), computed where the tensor leaves
//
// Return codes: see csp_io.h.

#include "csp_io.h"

#include <sys/mman.h>

extern "C" {

int csp_io_read_full(int fd, void* dst, size_t n, int timeout_ms) {
    return csp_io_detail::read_full(fd, dst, n, timeout_ms, nullptr);
}

int csp_io_write_full(int fd, const void* src, size_t n) {
    return csp_io_detail::write_full(fd, src, n, nullptr);
}

void* csp_io_alloc(size_t n) {
    if (n == 0) return nullptr;
    void* p = mmap(nullptr, n, PROT_READ | PROT_WRITE,
                   MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (p == MAP_FAILED) return nullptr;
#ifdef MADV_HUGEPAGE
    (void)madvise(p, n, MADV_HUGEPAGE);  // advice only: small pages still work
#endif
    return p;
}

int csp_io_free(void* p, size_t n) {
    if (!p || n == 0) return 0;
    return munmap(p, n) == 0 ? 0 : -errno;
}

// The loop is inlined here once per clone: the AVX2 one (picked at load time
// where the CPU has it) does four u32 x u32 -> u64 products per instruction,
// the baseline SSE2 one two.
#if defined(__x86_64__) && defined(__GNUC__) && !defined(__clang__)
__attribute__((target_clones("avx2", "default")))
#endif
void csp_io_checksum(const void* src, size_t n, uint64_t out[2]) {
    csp_io_detail::checksum(src, n, out);
}

}  // extern "C"
