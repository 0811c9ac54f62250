// The chores the host drivers share (tests/host_*_main.cpp, built by tests/host_program.py): buffers, typed files, the loop that stands
// for a workgroup's threads, and the pattern LDS holds before a workgroup starts.  A driver includes this first; PHASE takes THREADS from
// the core's namespace where it is used.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// n elements at a 16-byte boundary, `slack` bytes behind them: a core may load the 16 bytes that hold an input's last element
template <typename T>
static T* alloc16(size_t n, size_t slack = 16) {
    return (T*)aligned_alloc(16, (n * sizeof(T) + 15) / 16 * 16 + slack);
}

// the first n elements of a file in such a buffer; the program exits with 2 if they are not there
template <typename T>
static T* read_file(const char* path, size_t n, size_t slack = 16) {
    T* p = alloc16<T>(n, slack);
    FILE* fi = fopen(path, "rb");
    if (!fi || fread(p, sizeof(T), n, fi) != n) exit(2);
    fclose(fi);
    return p;
}

// 0, or 4 if the file cannot be written; n = 0 leaves an empty file
template <typename T>
static int write_file(const char* path, const T* p, size_t n) {
    FILE* fo = fopen(path, "wb");
    const bool ok = fo && (n == 0 || fwrite(p, sizeof(T), n, fo) == n);
    if (fo) fclose(fo);
    return ok ? 0 : 4;
}
template <typename T>
static int write_file(const char* path, const std::vector<T>& v) {
    return write_file(path, v.data(), v.size());
}

// one barrier-separated phase: `call` for thread t = 0 .. n - 1 of the workgroup, one after the other
#define PHASE_N(n, call) for (int t = 0; t < (n); ++t) { call; }
#define PHASE(call) PHASE_N(THREADS, call)

// LDS before a workgroup's first phase: a slot nobody wrote that reaches a result shows (NaN for a sum, a wild number for a counter)
template <typename T, typename V>
static void poison(T* lds, size_t n, const V& pattern) {
    for (size_t i = 0; i < n; ++i) lds[i] = pattern;
}
