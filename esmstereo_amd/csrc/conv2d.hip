// 2-D instantiations of the LDS-staged implicit-GEMM conv (see conv_impl.h).
#include "conv_impl.h"

namespace esm {

int launch_conv2d(const esm_conv_desc& a, hipStream_t s) {
    using namespace conv;
    if (a.transposed) return launch_geom<false, 4, 2, true>(a, s);
    const int k = a.kh, S = a.stride;
    if (k == 1 && S == 1) return launch_geom<false, 1, 1, false>(a, s);
    if (k == 3 && S == 1) return launch_geom<false, 3, 1, false>(a, s);
    if (k == 3 && S == 2) return launch_geom<false, 3, 2, false>(a, s);
    if (k == 5 && S == 1) return launch_geom<false, 5, 1, false>(a, s);
    set_error("conv2d: unsupported kernel/stride combination");
    return ESM_ERR_UNSUPPORTED;
}

int conv_check(const esm_conv_desc& a);  // conv.hip

}  // namespace esm

extern "C" int esm_convt_c1_ok(const esm_conv_desc* desc) {
    if (!desc) return esm::arg_error("conv: null descriptor");
    const int rc = esm::conv_check(*desc);
    return rc != ESM_OK ? rc : (esm::conv::convt_c1_ok(*desc) ? 1 : 0);
}

#ifdef ESM_CONV_STAMPS
// Diagnostic build only: copy out (and reset) the per-wave stamps of the 2-D direct kernels.
extern "C" int esm_diag_stamps(unsigned long long* host, int max_waves) {
    unsigned int n = 0;
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpyFromSymbol(&n, HIP_SYMBOL(esm::conv::esm_stamp_count), sizeof n) != hipSuccess)
        return -1;
    n = n < static_cast<unsigned>(max_waves) ? n : static_cast<unsigned>(max_waves);
    if (n && hipMemcpyFromSymbol(host, HIP_SYMBOL(esm::conv::esm_stamps), 8ull * n * sizeof(unsigned long long)) != hipSuccess)
        return -1;
    const unsigned int zero = 0;
    if (hipMemcpyToSymbol(HIP_SYMBOL(esm::conv::esm_stamp_count), &zero, sizeof zero) != hipSuccess) return -1;
    return static_cast<int>(n);
}
#endif
