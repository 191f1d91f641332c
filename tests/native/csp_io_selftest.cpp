// Stand-alone driver for ops/csrc/csp_io.cpp, meant to be compiled
// together with it under -fsanitize=address,undefined (see
// tests/test_native_io_sanitized.py).  It has its own main and runs as
// its own process; nothing here is ever loaded into Python.
//
// Exit status 0 = every check held; a failed check prints and exits 1; a
// sanitizer report aborts with its own status.

#include <cerrno>
#include <csignal>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include <fcntl.h>
#include <unistd.h>

extern "C" {
int csp_io_read_full(int fd, void* dst, size_t n, int timeout_ms);
int csp_io_write_full(int fd, const void* src, size_t n);
void* csp_io_alloc(size_t n);
int csp_io_free(void* p, size_t n);
}

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

static std::vector<unsigned char> pattern(size_t n) {
    std::vector<unsigned char> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = (unsigned char)((i * 7 + 3) % 251);
    return v;
}

static void set_nonblock(int fd) {
    int fl = fcntl(fd, F_GETFL);
    CHECK(fl >= 0 && fcntl(fd, F_SETFL, fl | O_NONBLOCK) == 0);
}

// writer thread -> pipe -> reader thread, both through the library, the
// destination sized exactly n so that one byte too many is a heap overflow
static void round_trip(size_t n, bool nonblock_r, bool nonblock_w) {
    int p[2];
    CHECK(pipe(p) == 0);
    if (nonblock_r) set_nonblock(p[0]);
    if (nonblock_w) set_nonblock(p[1]);
    std::vector<unsigned char> src = pattern(n);
    const char tail[] = "TAIL";
    std::thread w([&] {
        CHECK(csp_io_write_full(p[1], src.data(), n) == 0);
        CHECK(csp_io_write_full(p[1], tail, 4) == 0);
        close(p[1]);
    });
    unsigned char* dst = (unsigned char*)malloc(n ? n : 1);
    CHECK(csp_io_read_full(p[0], dst, n, 10000) == 0);
    CHECK(n == 0 || memcmp(dst, src.data(), n) == 0);
    char t[4];
    CHECK(csp_io_read_full(p[0], t, 4, 10000) == 0);  // nothing past n was taken
    CHECK(memcmp(t, tail, 4) == 0);
    char extra;
    CHECK(csp_io_read_full(p[0], &extra, 1, 10000) == 1);  // EOF
    w.join();
    free(dst);
    close(p[0]);
}

static void timeout_and_epipe() {
    int p[2];
    CHECK(pipe(p) == 0);
    char b[4];
    CHECK(csp_io_write_full(p[1], "ab", 2) == 0);
    CHECK(csp_io_read_full(p[0], b, 4, 30) == 2);  // 2 bytes, then timeout
    close(p[0]);
    std::vector<unsigned char> big = pattern(1 << 17);
    // SIGPIPE is at its default action here: it must not kill us
    CHECK(csp_io_write_full(p[1], big.data(), big.size()) == -EPIPE);
    close(p[1]);
    CHECK(csp_io_read_full(p[0], b, 1, 10) == -EBADF);
}

static void alloc_free() {
    const size_t n = (size_t(4) << 20) + 123;
    unsigned char* m = (unsigned char*)csp_io_alloc(n);
    CHECK(m != nullptr);
    CHECK(m[0] == 0 && m[n - 1] == 0);
    m[0] = 1;
    m[n - 1] = 2;
    CHECK(csp_io_free(m, n) == 0);
    CHECK(csp_io_alloc(0) == nullptr);
    CHECK(csp_io_free(nullptr, 0) == 0);
}

int main() {
    signal(SIGPIPE, SIG_DFL);
    const size_t sizes[] = {0, 1, 65535, 65537, (size_t(1) << 20) + 3};
    for (size_t n : sizes)
        for (int mode = 0; mode < 4; ++mode) round_trip(n, mode & 1, mode & 2);
    timeout_and_epipe();
    alloc_free();
    puts("csp_io selftest ok");
    return 0;
}
