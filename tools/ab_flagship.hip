// ab_flagship.hip -- A/B harness for variants of the flagship min-sum body (ldpc_spec::ms_m64_body) on the shipped example code:
// every variant decodes the SAME 65536 frames (Eb/N0 0 dB: all 50 iterations run), outputs are compared bit for bit with the
// baseline, rounds are interleaved in one process (guide rule 24).  Build: hipcc --offload-arch=gfx950 -O3 -std=c++17
// -ffp-contract=off tools/ab_flagship.hip -o tools/ab_flagship.bin.   usage: ab_flagship.bin [frames] [Eb/N0 dB] [rounds]
// Results: profiles/r06_flagship_variants.txt (round 2's variants -- the record word, the exec-masked dual ds_add -- are in
// profiles/r02_flagship_variants.txt; the record word is part of every body here).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../ldpc-lib_amd/csrc/ldpc_spec.hpp"
#include "../ldpc-lib_amd/csrc/code_appendix_c_m64.hpp"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

namespace ldpc_spec {

// The body with this round's changes behind flags; ms_m64_body_x<C, false, false> is the body as it was before round 6, word for word
// (one workgroup per frame: no frame queue here).
//   UNWRAP  the frame's image starts 512 B into the LDS allocation (the launch passes 8 N + 512 bytes).  Variable (lane + c) mod 64
//           of block column k is then at  base + 512 k + 8 c  with  base = lane + c >= 64 ? lds + 8 lane : lds + 8 lane + 512:
//           one select under a compile-time lane mask between two long-lived address registers, the rest in the instruction's
//           offset field -- instead of add, and, add-the-LDS-base (three VOP2) per rotated edge and a copy + add per block row.
//   FOLD0   slot 0 of STATE3 starts from nm1 = nm2 = MAX_VAL, npos = 0:  nm2 = min(max(v, K), K) = K and npos = sel(0, 0) = 0
//           whatever v is, so slot 0 is nm1 = min(v, K) alone (max, min, compare and select fewer per block row).
template <class C, bool UNWRAP, bool FOLD0>
__device__ __forceinline__ void ms_m64_body_x(const SpecArgs &a) {
    static_assert(C::M == 64, "one frame per wavefront needs M == 64");
    constexpr int RH = C::RH, NH = C::NH, N = C::NH * 64;
    extern __shared__ double lds[];
    char *const ldsb = reinterpret_cast<char *>(lds);
    const int lane = threadIdx.x;
    const u32 n8 = (u32)lane * 8u;
    const double alpha = a.alpha;
    const long long fr = blockIdx.x;
    // UNWRAP: LDS addresses of this lane's variable one row below the image (lo: lanes that wrap) and inside it (hi)
    const u32 lo = lds_addr(lds) + n8, hi = lo + 512u;
    auto rot = [&](u32 base, auto S) -> u32 {
        constexpr int c = decltype(S)::value;
        if constexpr (c == 0) return base;
        else return (base + 8u * (u32)c) & 511u;
    };
    // address of variable (lane + c) mod 64 of block column k; `tie`: see sel32_tied in ldpc_spec.hpp
    auto at = [&](u32 nb, u32 tie, auto S, auto K) -> double * {
        constexpr int c = decltype(S)::value, k = decltype(K)::value;
        if constexpr (!UNWRAP) return reinterpret_cast<double *>(ldsb + rot(nb, S) + k * 512);
        else if constexpr (c == 0) return lds_at(hi + (u32)(k * 512));
        else return lds_at(sel32_tied(hi, lo, ~0ull << (64 - c), tie) + (u32)(k * 512 + 8 * c));
    };
    auto own = [&](auto K) -> double * {   // this lane's own variable of block column k
        constexpr int k = decltype(K)::value;
        if constexpr (!UNWRAP) return reinterpret_cast<double *>(ldsb + n8 + k * 512);
        else return lds_at(hi + (u32)(k * 512));
    };
    const double *const yrow = a.llr + fr * N + lane;
    double m1[RH], m2[RH];
    u32 meta[RH];  // [31:32-RW] sign of the c2v on slot s (own v2c sign xor row sign) on bit 31-s; [7:0] slot of the min1 edge
    static_for<0, RH>([&](auto J) { constexpr int j = decltype(J)::value; m1[j] = 0.0; m2[j] = 0.0; meta[j] = 0u; });

    int res = -a.maxiter;
    for (int iter = 0; iter < a.maxiter; ++iter) {
        double y[NH];
        int yo = 0;
        asm volatile("" : "+v"(yo));
        static_for<0, NH>([&](auto K) { constexpr int k = decltype(K)::value; y[k] = yrow[yo + k * 64]; });
        // ---------------- STATE1
        static_for<0, RH>([&](auto J) {
            constexpr int j = decltype(J)::value;
            u32 mt = meta[j], nb = n8;
            if constexpr (UNWRAP) asm volatile("" : "+v"(mt));
            else asm volatile("" : "+v"(mt), "+v"(nb));
            const u32 pos = mt & 0xffu;
            u32 Wt = mt;
            static_for<0, C::RW[j]>([&](auto S) {
                constexpr int s = decltype(S)::value;
                const double aa = sel64(m1[j], m2[j], lanes_eq(pos, (u32)s));
                const double cv = signed_mag(aa, Wt);
                Wt = twice(Wt);
                double *p = at(nb, mt, IC<C::SH[j][s]>{}, IC<C::COL[j][s]>{});
                if constexpr (C::FIRST[j][s]) *p = cv;
                else __hip_atomic_fetch_add(p, cv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            });
            __builtin_amdgcn_sched_barrier(0);
        });
        // ---------------- STATE2
        static_for<0, NH>([&](auto K) {
            constexpr int k = decltype(K)::value;
            double *p = own(K);
            const double pr = *p * alpha;
            *p = (y[k] + 0.0) + pr;
            if constexpr (k % 8 == 7) __builtin_amdgcn_sched_barrier(0);
        });
        // ---------------- STATE3
        u32 failw = 0;
        static_for<0, RH>([&](auto J) {
            constexpr int j = decltype(J)::value;
            constexpr int RW = C::RW[j];
            u32 mt = meta[j];
            asm volatile("" : "+v"(mt));
            const u32 pos = mt & 0xffu;
            u32 Wt = mt;
            double a1 = m1[j] * alpha, a2 = m2[j] * alpha;
            asm volatile("" : "+v"(a1), "+v"(a2));
            double nm1 = kMaxVal, nm2 = kMaxVal;
            u32 npos = 0, nS = 0, sy = 0;
            u32 nb = n8;
            if constexpr (!UNWRAP) asm volatile("" : "+v"(nb));
            double r[RW];
            static_for<0, RW>([&](auto S) {
                constexpr int s = decltype(S)::value;
                r[s] = *at(nb, mt, IC<C::SH[j][s]>{}, IC<C::COL[j][s]>{});
            });
            static_for<0, RW>([&](auto S) {
                constexpr int s = decltype(S)::value;
                sy ^= hi32(r[s]);
                const double aa = sel64(a1, a2, lanes_eq(pos, (u32)s));
                const double x = signed_mag(aa, Wt);
                Wt = twice(Wt);
                const double tt = r[s] - x;
                nS = __builtin_amdgcn_alignbit(nS, hi32(tt), 31);
                const double v = fabs(tt);
                if constexpr (FOLD0 && s == 0) {
                    nm1 = fmin(v, kMaxVal);
                } else {
                    const mask64 c1 = lanes_lt(v, nm1);
                    nm2 = fmin(fmax(v, nm1), nm2);
                    npos = sel32(npos, (u32)s, c1);
                    nm1 = fmin(v, nm1);
                }
            });
            failw |= sy;
            const u32 w = (nS ^ (0u - (__popc(nS) & 1u))) << (32 - RW);
            m1[j] = nm1; m2[j] = nm2; meta[j] = w | npos;
            __builtin_amdgcn_sched_barrier(0);
        });
        if (__ballot((failw >> 31) != 0) == 0ull) { res = iter + 1; break; }
    }
    if (lane == 0 && a.iters) a.iters[fr] = res;
    if (a.hard) {
        u64 mine = 0ull;
        static_for<0, NH>([&](auto K) {
            constexpr int k = decltype(K)::value;
            const u64 b = __ballot((hi32(*own(K)) >> 31) != 0);
            if (lane == k) mine = b;
        });
        if (lane < NH) reinterpret_cast<u64 *>(a.hard + fr * (N / 32))[lane] = mine;
    }
    if (a.soft_out) {
        static_for<0, NH>([&](auto K) {
            constexpr int k = decltype(K)::value;
            a.soft_out[fr * N + k * 64 + lane] = *own(K);
        });
    }
}

}  // namespace ldpc_spec

using ldpc_spec::SpecArgs;
typedef ldpc_spec::CodeAppendixCM64 Code;
__global__ void __launch_bounds__(64, 2) k_parent(const SpecArgs a) { ldpc_spec::ms_m64_body_x<Code, false, false>(a); }
__global__ void __launch_bounds__(64, 2) k_unwrap(const SpecArgs a) { ldpc_spec::ms_m64_body_x<Code, true, false>(a); }
__global__ void __launch_bounds__(64, 2) k_fold0(const SpecArgs a) { ldpc_spec::ms_m64_body_x<Code, false, true>(a); }
__global__ void __launch_bounds__(64, 2) k_both(const SpecArgs a) { ldpc_spec::ms_m64_body_x<Code, true, true>(a); }
__global__ void __launch_bounds__(64, 2) k_shipped(const SpecArgs a) { ldpc_spec::ms_m64_body<Code>(a); }

struct Variant { const void *kern; const char *name; size_t lds; };

int main(int argc, char **argv) {
    const long long B = argc > 1 ? atoll(argv[1]) : 65536;
    const double snr = argc > 2 ? atof(argv[2]) : 0.0;
    const int rounds = argc > 3 ? atoi(argv[3]) : 8;
    const int N = 2048;
    const Variant var[] = {
        {(const void *)k_parent, "baseline: the body before round 6", (size_t)N * 8},
        {(const void *)k_unwrap, "1b: image 512 B into the allocation, one select per rotated edge", (size_t)N * 8 + 512},
        {(const void *)k_fold0, "2: slot 0 of STATE3 folded (nm2 = K, npos = 0)", (size_t)N * 8},
        {(const void *)k_both, "1b + 2", (size_t)N * 8 + 512},
        {(const void *)k_shipped, "ms_m64_body as shipped (ldpc_spec.hpp; 1b + 2, frame loop)", ldpc_spec::kMsM64LdsBytes(N)},
    };
    constexpr int NV = sizeof var / sizeof var[0];
    const long long distinct = std::min<long long>(B, 4096);
    std::vector<double> h((size_t)distinct * N);
    std::mt19937_64 g(1);
    std::normal_distribution<double> nd;
    const double sigma = std::sqrt(std::pow(10, -snr / 10) / 2 / 0.5);
    for (auto &v : h) v = -2.0 * (sigma * nd(g) - 1.0) / (sigma * sigma);
    double *d_llr, *d_soft[NV];
    unsigned *d_hard[NV];
    int *d_it[NV];
    CK(hipMalloc(&d_llr, sizeof(double) * (size_t)B * N));
    for (long long f = 0; f < B; f += distinct)
        CK(hipMemcpy(d_llr + (size_t)f * N, h.data(), sizeof(double) * (size_t)std::min(distinct, B - f) * N, hipMemcpyHostToDevice));
    for (int v = 0; v < NV; ++v) {
        CK(hipMalloc(&d_soft[v], sizeof(double) * (size_t)4096 * N));
        CK(hipMalloc(&d_hard[v], 4 * (size_t)B * (N / 32)));
        CK(hipMalloc(&d_it[v], 4 * (size_t)B));
    }
    std::vector<float> best(NV, 1e9f), worst(NV, 0.f), sum(NV, 0.f);
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (int r = 0; r <= rounds; ++r)   // round 0 warms up
        for (int v = 0; v < NV; ++v) {
            SpecArgs a{};
            a.llr = d_llr; a.hard = d_hard[v]; a.iters = d_it[v]; a.soft_out = nullptr; a.maxiter = 50; a.alpha = 0.8; a.nframes = B;
            void *args[] = {&a};
            CK(hipEventRecord(e0, 0));
            CK(hipLaunchKernel(var[v].kern, dim3((unsigned)B), dim3(64), args, var[v].lds, 0));
            CK(hipEventRecord(e1, 0));
            CK(hipEventSynchronize(e1));
            float ms;
            CK(hipEventElapsedTime(&ms, e0, e1));
            if (r) { best[v] = std::min(best[v], ms); worst[v] = std::max(worst[v], ms); sum[v] += ms; }
        }
    // soft values on the first 4096 frames + bitwise comparison with the baseline
    std::vector<unsigned> hh[NV];
    std::vector<int> hi[NV];
    std::vector<double> hs[NV];
    for (int v = 0; v < NV; ++v) {
        SpecArgs a{};
        a.llr = d_llr; a.hard = nullptr; a.iters = nullptr; a.soft_out = d_soft[v]; a.maxiter = 50; a.alpha = 0.8; a.nframes = 4096;
        void *args[] = {&a};
        CK(hipLaunchKernel(var[v].kern, dim3(4096), dim3(64), args, var[v].lds, 0));
        CK(hipDeviceSynchronize());
        hh[v].resize((size_t)B * (N / 32)); hi[v].resize((size_t)B); hs[v].resize((size_t)4096 * N);
        CK(hipMemcpy(hh[v].data(), d_hard[v], 4 * hh[v].size(), hipMemcpyDeviceToHost));
        CK(hipMemcpy(hi[v].data(), d_it[v], 4 * hi[v].size(), hipMemcpyDeviceToHost));
        CK(hipMemcpy(hs[v].data(), d_soft[v], 8 * hs[v].size(), hipMemcpyDeviceToHost));
    }
    double mean_it = 0;
    for (int x : hi[0]) mean_it += std::abs(x);
    mean_it /= (double)B;
    printf("# %lld frames, Eb/N0 %.1f dB, mean |iters| %.2f, %d interleaved rounds; spread = max - min over the rounds\n", B, snr, mean_it, rounds);
    for (int v = 0; v < NV; ++v) {
        const bool same = hh[v] == hh[0] && hi[v] == hi[0] && !memcmp(hs[v].data(), hs[0].data(), 8 * hs[0].size());
        printf("%-68s min %8.3f ms  mean %8.3f ms  max %8.3f ms  spread %5.2f %%  %6.3f Mframes/s  outputs %s\n", var[v].name, best[v],
               sum[v] / rounds, worst[v], 100.0 * (worst[v] - best[v]) / best[v], B / best[v] / 1e3,
               same ? "bit-identical to the baseline" : "DIFFER");
    }
    return 0;
}
