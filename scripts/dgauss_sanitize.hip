// Stand-alone host program over the discrete Gaussian sampler (csrc/kernels.hpp: dgauss_run, dgauss_sample, DgSeeded), for a sanitizer run
// of the host side only -- no GPU is touched, no device code is instrumented:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -DROFL_FD_CHECK_HOST -Irofl_project_code_amd/csrc \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined scripts/dgauss_sanitize.hip -o scripts/dgauss_sanitize \
//         -fsanitize=address,undefined && scripts/dgauss_sanitize
// 20 000 elements of seed 00 01 .. 1f at nine sigma2 through the on-demand source (the host twin's), each again over a plain buffer of
// exactly the words it used (equal) and of one word less (not finished), then the dry, the all-ones and the empty list.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <vector>
#define ROFL_KGROUP -1
#include "kernels.hpp"
using namespace rofl;
int main() {
    uint8_t seed[32]; for (int i = 0; i < 32; i++) seed[i] = (uint8_t)i;
    u64 sd[4]; memcpy(sd, seed, 32);
    long long sum = 0; unsigned maxused = 0;
    const u32 s2s[] = {1, 2, 3, 15, 16, 50, 4096, 1u << 16, 1u << 24};
    for (u32 s2 : s2s)
        for (u64 e = 0; e < 20000; e++) {
            u32 blk[32];
            DgSeeded src{sd[0], sd[1], sd[2], sd[3], e, blk, ~0u, 0};
            DgaussOut r = dgauss_run(src, s2);
            // the same element over a plain buffer of exactly the words it used, and one short
            std::vector<u32> w;
            for (u32 j = 0; j < (r.used + 31) / 32; j++) { u32 b[32]; dg_squeeze(b, sd[0], sd[1], sd[2], sd[3], e, j); w.insert(w.end(), b, b + 32); }
            w.resize(r.used);
            DgaussOut a = dgauss_sample(w.data(), (u32)w.size(), s2);
            if (!a.finished || a.noise != r.noise || a.used != r.used) { printf("MISMATCH %u %llu\n", s2, (unsigned long long)e); return 1; }
            if (r.used) { w.resize(r.used - 1); DgaussOut c = dgauss_sample(w.data(), (u32)w.size(), s2); if (c.finished) { printf("SHORT FINISHED\n"); return 1; } }
            sum += r.noise; if (r.used > maxused) maxused = r.used;
        }
    std::vector<u32> z(8192, 0), f(8192, 0xffffffffu);
    DgaussOut a = dgauss_sample(z.data(), 8192, 1), b = dgauss_sample(f.data(), 8192, 1), c = dgauss_sample(nullptr, 0, 1);
    printf("sum %lld maxused %u | zeros %u %d %u | ff %u %d %u | empty %u %d %u\n", sum, maxused, a.finished, a.noise, a.used, b.finished, b.noise, b.used, c.finished, c.noise, c.used);
    return 0;
}
