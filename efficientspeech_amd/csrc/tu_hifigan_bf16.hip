// esmi C-ABI, translation unit "tu_hifigan_bf16.hip": the one-launch ResBlock kernels of the HiFi-GAN generator at bf16
// (hifigan_resblock.h: one bfloat16 product per contraction, ESMI_PRECISION_BF16).  A unit of its own: its twelve instantiations compile
// beside tu_hifigan.hip's and tu_hifigan_amp.hip's instead of behind them.  The generator's host side (tu_hifigan.hip) decides when they run.
// One of several translation units of libesmi.so (compiled in parallel by __graft_entry__.build(); the simulator build
// tools/wavesim/build.sh compiles the same files with the host compiler).  Internal launchers are declared in launch.h.
#include "launch.h"

using namespace esmi;
ESMI_TU_RANGE_SETTER(hifigan_bf16)

namespace esmi {

#if ESMI_CHAIN_SPLIT
template <int C, int K>
int launch_resblock_bf16_ck(const ResblockP& p, hipStream_t st) {
    const size_t lds = rb_amp_lds_bytes(C, p.R);
    const dim3 grid((unsigned)(p.B * p.tiles_per_b));
    if (p.R > rb_amp_rmax(C)) return ESMI_ERR_ARG;   // (rows past the waves' items would never be computed)
    if constexpr (C <= 16) {   // narrow MFMA tiles (16 channels x 16 positions): LDS <= 16 KB
        ESMI_LAUNCH((hifigan_resblock16_bf16_kernel<C, K>), grid, dim3(64 * kRbWaves), lds, st, p);
    } else {
        static AttrOnce once;
        if (lds > 48 * 1024)
            if (int rc = raise_lds_limit(reinterpret_cast<const void*>(hifigan_resblock_bf16_kernel<C, K>), once)) return rc;
        ESMI_LAUNCH((hifigan_resblock_bf16_kernel<C, K>), grid, dim3(64 * rb_amp_waves(C)), lds, st, p);
    }
    return launch_status();
}
template <int C>
int launch_resblock_bf16_c(const ResblockP& p, hipStream_t st) {
    switch (p.k) {
        case 3: return launch_resblock_bf16_ck<C, 3>(p, st);
        case 7: return launch_resblock_bf16_ck<C, 7>(p, st);
        case 11: return launch_resblock_bf16_ck<C, 11>(p, st);
    }
    return ESMI_ERR_UNSUPPORTED;
}
int launch_resblock_bf16(const ResblockP& p, int c, hipStream_t st) {
    switch (c) {
        case 8: return launch_resblock_bf16_c<8>(p, st);
        case 16: return launch_resblock_bf16_c<16>(p, st);
        case 32: return launch_resblock_bf16_c<32>(p, st);
        case 64: return launch_resblock_bf16_c<64>(p, st);
    }
    return ESMI_ERR_UNSUPPORTED;
}
#else
int launch_resblock_bf16(const ResblockP&, int, hipStream_t) { return ESMI_ERR_UNSUPPORTED; }   // the exact-fp32 build has no one-product path
#endif

}  // namespace esmi
