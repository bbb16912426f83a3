// math_probe.hip -- evaluates the device math functions of ldpc_spec.hpp elementwise on a GPU, for tests/test_gpu_device_math.py.
//
//   math_probe <op> <in.bin> <out.bin>
//
// Files: a header of two little-endian u64 (element count n, number of arrays k), then k arrays of n 8-byte elements each.
//   op       in              out
//   exp      x               exp_glibc(x)
//   expw     x               exp_glibc_wide(x, kExpTab)
//   log      x               log_glibc(x)
//   div      a, b            div_ranged(a, b), a / b
//   sqrt     x               sqrt(x)
//   phi      x               lche::logexp(x, kLcheTab, kLcheStep), tables in global memory
//   phi_lds  x               the same, both tables copied to LDS first (as lche_body does)
//   prior    x               iasp::prior(x), iasp::q12 of it (as u64)
// One grid-stride kernel per op, arrays in, arrays out.  Built with the library's flags (binding.HIPCC_FLAGS), so what it
// evaluates is what the decoders evaluate.  phi / phi_lds must not be given NaN (the table index is derived from the operand).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../ldpc-lib_amd/csrc/ldpc_spec.hpp"
#include "../../ldpc-lib_amd/csrc/lche_table.hpp"

namespace {

constexpr unsigned long long kMaxElems = 1ull << 20;
constexpr int kThreads = 256, kBlocks = 256;

#define PROBE_HIP(call)                                                                                         \
    do {                                                                                                        \
        const hipError_t e_ = (call);                                                                           \
        if (e_ != hipSuccess) {                                                                                 \
            std::fprintf(stderr, "math_probe: %s: %s (%s:%d)\n", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return 1;                                                                                           \
        }                                                                                                       \
    } while (0)

#define PROBE_LOOP for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)

__global__ void exp_kernel(const double *x, double *y, size_t n) { PROBE_LOOP y[i] = ldpc_spec::exp_glibc(x[i]); }
__global__ void expw_kernel(const double *x, double *y, size_t n) { PROBE_LOOP y[i] = ldpc_spec::exp_glibc_wide(x[i], ldpc_spec::kExpTab); }
__global__ void log_kernel(const double *x, double *y, size_t n) { PROBE_LOOP y[i] = ldpc_spec::log_glibc(x[i]); }
__global__ void div_kernel(const double *a, const double *b, double *q, double *qc, size_t n) {
    PROBE_LOOP {
        q[i] = ldpc_spec::div_ranged(a[i], b[i]);
        qc[i] = a[i] / b[i];
    }
}
__global__ void sqrt_kernel(const double *x, double *y, size_t n) { PROBE_LOOP y[i] = sqrt(x[i]); }
__global__ void phi_kernel(const double *x, double *y, size_t n) {
    PROBE_LOOP y[i] = ldpc_spec::lche::logexp(x[i], ldpc_spec::lche::kLcheTab, ldpc_spec::lche::kLcheStep);
}
__global__ void phi_lds_kernel(const double *x, double *y, size_t n) {
    __shared__ double tab[ldpc_spec::lche::kTabWords + ldpc_spec::lche::kStepWords];
    for (int i = threadIdx.x; i < ldpc_spec::lche::kTabWords + ldpc_spec::lche::kStepWords; i += blockDim.x)
        tab[i] = i < ldpc_spec::lche::kTabWords ? ldpc_spec::lche::kLcheTab[i] : ldpc_spec::lche::kLcheStep[i - ldpc_spec::lche::kTabWords];
    __syncthreads();
    const double *const T = tab, *const S = tab + ldpc_spec::lche::kTabWords;
    PROBE_LOOP y[i] = ldpc_spec::lche::logexp(x[i], T, S);
}
__global__ void prior_kernel(const double *x, double *p, unsigned long long *q, size_t n) {
    PROBE_LOOP {
        const double v = ldpc_spec::iasp::prior(x[i]);
        p[i] = v;
        q[i] = ldpc_spec::iasp::q12(v);
    }
}

struct Op { const char *name; int nin, nout; };
const Op kOps[] = {{"exp", 1, 1}, {"expw", 1, 1}, {"log", 1, 1}, {"div", 2, 2}, {"sqrt", 1, 1}, {"phi", 1, 1}, {"phi_lds", 1, 1}, {"prior", 1, 2}};

}  // namespace

int main(int argc, char **argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: math_probe <op> <in.bin> <out.bin>\n");
        return 2;
    }
    const Op *op = nullptr;
    for (const Op &o : kOps)
        if (!std::strcmp(o.name, argv[1])) op = &o;
    if (!op) {
        std::fprintf(stderr, "math_probe: unknown op %s\n", argv[1]);
        return 2;
    }
    std::FILE *f = std::fopen(argv[2], "rb");
    if (!f) {
        std::fprintf(stderr, "math_probe: cannot open %s\n", argv[2]);
        return 2;
    }
    unsigned long long hdr[2] = {0, 0};
    if (std::fread(hdr, 8, 2, f) != 2 || hdr[0] == 0 || hdr[0] > kMaxElems || hdr[1] != (unsigned long long)op->nin) {
        std::fprintf(stderr, "math_probe: %s: bad header (1 <= n <= 2^20 and %d arrays expected)\n", argv[2], op->nin);
        std::fclose(f);
        return 2;
    }
    const size_t n = (size_t)hdr[0];
    std::vector<unsigned long long> in(n * op->nin), out(n * op->nout);
    const bool whole = std::fread(in.data(), 8, in.size(), f) == in.size();
    std::fclose(f);
    if (!whole) {
        std::fprintf(stderr, "math_probe: %s is shorter than its header says\n", argv[2]);
        return 2;
    }

    unsigned long long *din = nullptr, *dout = nullptr;
    PROBE_HIP(hipMalloc(&din, in.size() * 8));
    PROBE_HIP(hipMalloc(&dout, out.size() * 8));
    PROBE_HIP(hipMemcpy(din, in.data(), in.size() * 8, hipMemcpyHostToDevice));
    PROBE_HIP(hipMemset(dout, 0xff, out.size() * 8));
    const double *x = reinterpret_cast<const double *>(din);
    double *y = reinterpret_cast<double *>(dout);
    const std::string name = op->name;
    if (name == "exp") exp_kernel<<<kBlocks, kThreads>>>(x, y, n);
    else if (name == "expw") expw_kernel<<<kBlocks, kThreads>>>(x, y, n);
    else if (name == "log") log_kernel<<<kBlocks, kThreads>>>(x, y, n);
    else if (name == "div") div_kernel<<<kBlocks, kThreads>>>(x, x + n, y, y + n, n);
    else if (name == "sqrt") sqrt_kernel<<<kBlocks, kThreads>>>(x, y, n);
    else if (name == "phi") phi_kernel<<<kBlocks, kThreads>>>(x, y, n);
    else if (name == "phi_lds") phi_lds_kernel<<<kBlocks, kThreads>>>(x, y, n);
    else prior_kernel<<<kBlocks, kThreads>>>(x, y, dout + n, n);
    PROBE_HIP(hipGetLastError());
    PROBE_HIP(hipDeviceSynchronize());
    PROBE_HIP(hipMemcpy(out.data(), dout, out.size() * 8, hipMemcpyDeviceToHost));
    PROBE_HIP(hipFree(din));
    PROBE_HIP(hipFree(dout));

    f = std::fopen(argv[3], "wb");
    const unsigned long long ohdr[2] = {(unsigned long long)n, (unsigned long long)op->nout};
    if (!f || std::fwrite(ohdr, 8, 2, f) != 2 || std::fwrite(out.data(), 8, out.size(), f) != out.size() || std::fclose(f) != 0) {
        std::fprintf(stderr, "math_probe: cannot write %s\n", argv[3]);
        return 2;
    }
    return 0;
}
