// aot/lche.hip -- ahead-of-time instances (ldpc_aot.hpp), one translation unit of the parallel build
#include "../ldpc_aot.hpp"

// two lanes per check: 2 M threads per frame, two waves per SIMD
LDPC_AOT_KERNEL(lche_spec_appendix_c_m64_kernel, lche_body, CodeAppendixCM64, 128, 2)
