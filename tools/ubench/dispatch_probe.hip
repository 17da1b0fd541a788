// Launch-floor probe (development tool): what a launch of N one-wave items costs when the waves do nothing -- lane 0 of each wave
// stores one double -- by workgroup size (64 / 128 / 256 threads), dynamic LDS per wave (0 or pk_pat_lds_bytes(413) = 3592 bytes),
// private segment (off, or forced on by a nine-word local array that no wave touches at run time) and the register bounds of
// pk_rank_merge_nostore (amdgpu_waves_per_eu(7, 8), 64 VGPRs).  Grids of 2 048, 20 480 and 40 960 waves, the launch sizes of the
// committed merge measurements.  hipEvents around every launch, median / min of REPS launches after warm-up, one JSON line per shape.
// No spins, no communication between workgroups.
// hipcc --offload-arch=gfx950 -O3 -o /tmp/dispatch_probe tools/ubench/dispatch_probe.hip && /tmp/dispatch_probe profiles/dispatch_probe.jsonl
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

// `never` is 0 at run time: the array is there for the descriptor alone (volatile: the compiler may not promote it to registers)
template <int NT, bool PRIV>
__device__ __forceinline__ void probe_body(double* out, int n, int never) {
    const int item = (int)blockIdx.x * (NT / 64) + (int)(threadIdx.x >> 6);
    if (item >= n) return;
    double v = 1.0;
    if constexpr (PRIV) {
        if (never != 0) {
            volatile int loc[9];
            for (int i = 0; i < 9; ++i) loc[i] = i * never;
            v = (double)loc[(unsigned)never % 9u];
        }
    }
    if ((threadIdx.x & 63) == 0) out[item] = v;
}
template <int NT, bool PRIV>
__global__ __launch_bounds__(NT) void probe_plain(double* out, int n, int never) { probe_body<NT, PRIV>(out, n, never); }
template <int NT, bool PRIV>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(7, 8), amdgpu_num_vgpr(32)))
void probe_bounds(double* out, int n, int never) { probe_body<NT, PRIV>(out, n, never); }

typedef void (*probe_fn)(double*, int, int);
template <int NT>
static probe_fn pick(bool priv, bool bounds) {
    if (bounds) return priv ? probe_bounds<NT, true> : probe_bounds<NT, false>;
    return priv ? probe_plain<NT, true> : probe_plain<NT, false>;
}

int main(int argc, char** argv) {
    const int REPS = 60, WARM = 10, NMAX = 40960;
    FILE* f = argc > 1 ? fopen(argv[1], "w") : nullptr;
    if (argc > 1 && !f) { fprintf(stderr, "cannot write %s\n", argv[1]); return 1; }
    double* out = nullptr;
    CHECK(hipMalloc(&out, (size_t)NMAX * sizeof(double)));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    hipStream_t st;
    CHECK(hipStreamCreate(&st));
    const int grids[3] = {2048, 20480, NMAX}, nts[3] = {64, 128, 256};
    const size_t lds_wave[2] = {0, 3592};
    std::vector<double> host(NMAX);
    for (int n : grids)
        for (int nt : nts)
            for (size_t lw : lds_wave)
                for (int priv = 0; priv < 2; ++priv)
                    for (int bounds = 0; bounds < 2; ++bounds) {
                        probe_fn k = nt == 64 ? pick<64>(priv, bounds) : nt == 128 ? pick<128>(priv, bounds) : pick<256>(priv, bounds);
                        const int W = nt / 64, wgs = (n + W - 1) / W;
                        const size_t lds = lw * W;
                        CHECK(hipMemsetAsync(out, 0, (size_t)NMAX * sizeof(double), st));
                        std::vector<float> us;
                        for (int it = 0; it < WARM + REPS; ++it) {
                            hipExtLaunchKernelGGL(k, dim3(wgs), dim3(nt), lds, st, e0, e1, 0, out, n, 0);
                            CHECK(hipGetLastError());
                            CHECK(hipEventSynchronize(e1));
                            float ms = 0;
                            CHECK(hipEventElapsedTime(&ms, e0, e1));
                            if (it >= WARM) us.push_back(ms * 1000.0f);
                        }
                        CHECK(hipMemcpy(host.data(), out, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
                        int bad = 0;
                        for (int i = 0; i < n; ++i) bad += host[i] != 1.0;
                        std::sort(us.begin(), us.end());
                        char line[512];
                        snprintf(line, sizeof line,
                                 "{\"waves\": %d, \"threads\": %d, \"workgroups\": %d, \"lds_per_wave\": %zu, \"private_segment\": %d, "
                                 "\"merge_bounds\": %d, \"reps\": %d, \"median_us\": %.3f, \"min_us\": %.3f, \"p90_us\": %.3f, \"wrong\": %d}",
                                 n, nt, wgs, lw, priv, bounds, REPS, us[us.size() / 2], us[0], us[us.size() * 9 / 10], bad);
                        puts(line);
                        if (f) { fputs(line, f); fputc('\n', f); fflush(f); }
                        if (bad) { fprintf(stderr, "wrong output\n"); return 2; }
                    }
    if (f) fclose(f);
    CHECK(hipFree(out));
    return 0;
}
