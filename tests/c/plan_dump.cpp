// Host-only listing of a `.bcplan` through the parser of blobctrl_amd/csrc/plan_format.h (the one bc_plan_load uses), for tests that
// check WHAT a compiled plan launches without a GPU:  g++ -std=c++17 plan_dump.cpp
// usage: plan_dump FILE  - prints
//   buf <index> <name or -> <bytes>
//   seg <name> <launches>
//   rec <op> <sid> <arg>...     (non-GEMM launches; pointer = p<buffer index>+<byte offset> or p-, int / long = decimal, float = %.9g)
// or "rejected: <reason>" (exit status 1).
#include <stdlib.h>
#include "../../blobctrl_amd/csrc/plan_format.h"

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s plan.bcplan\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { printf("rejected: cannot open\n"); return 1; }
    bcplan::PlanImage img;
    char* arena = nullptr;
    uint64_t arena_bytes = 0;
    const std::string why = bcplan::parse_plan(
        f, img,
        [&](uint64_t bytes) -> uint64_t {
            if (bytes > (1ull << 32)) return 0;
            arena = static_cast<char*>(calloc(1, (size_t)bytes));
            arena_bytes = bytes;
            return (uint64_t)(uintptr_t)arena;
        },
        [&](uint64_t off, const char* host, size_t n) {
            if (off + n > arena_bytes) return false;
            memcpy(arena + off, host, n);
            return true;
        });
    fclose(f);
    if (!why.empty()) { printf("rejected: %s\n", why.c_str()); free(arena); return 1; }
    for (size_t i = 0; i < img.bufs.size(); ++i)
        printf("buf %zu %s %llu\n", i, img.bufs[i].name.empty() ? "-" : img.bufs[i].name.c_str(), (unsigned long long)img.bufs[i].bytes);
    auto where = [&](uint64_t addr) {
        if (!addr) { printf(" p-"); return; }
        // the buffer that holds the address; one-past-the-end of a buffer only when no buffer starts there (buffers are adjacent)
        for (int end_ok = 0; end_ok < 2; ++end_ok)
            for (size_t i = 0; i < img.bufs.size(); ++i)
                if (addr >= img.bufs[i].addr && (addr < img.bufs[i].addr + img.bufs[i].bytes ||
                                                 (end_ok && addr == img.bufs[i].addr + img.bufs[i].bytes))) {
                    printf(" p%zu+%llu", i, (unsigned long long)(addr - img.bufs[i].addr));
                    return;
                }
        printf(" p?");
    };
    for (auto& s : img.segs) {
        printf("seg %s %zu\n", s.name.c_str(), s.recs.size());
        for (auto& r : s.recs) {
            if (r.op == BC_OP_GEMM) { printf("rec %d %d\n", r.op, r.sid); continue; }
            printf("rec %d %d", r.op, r.sid);
            const char* sig = bcplan::op_signature(r.op);
            for (size_t k = 0; k < r.a.size(); ++k) {
                if (sig[k] == 'p') where(r.a[k]);
                else if (sig[k] == 'f') { const uint32_t u = (uint32_t)r.a[k]; float v; memcpy(&v, &u, 4); printf(" %.9g", (double)v); }
                else printf(" %lld", (long long)(int64_t)r.a[k]);
            }
            printf("\n");
        }
    }
    free(arena);
    return 0;
}
