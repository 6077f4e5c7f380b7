// esmi C-ABI, translation unit "tu_convgemm_bf16.hip": the implicit-GEMM families of convgemm.h / pwgemm.h with bfloat16 operands
// (ConvGemmP::amp == 2: the training step's bf16-mixed precision and the generator at bf16, ESMI_PRECISION_BF16).  launch_convgemm (tu_convgemm.hip) picks the
// family, the tiling and the grid; the launchers below only select the instantiation.  A unit of its own so that the cold build
// compiles these instantiations next to the binary16 ones, not after them.
// One of several translation units of libesmi.so (compiled in parallel by __graft_entry__.build(); the simulator build
// tools/wavesim/build.sh compiles the same files with the host compiler).  Internal launchers are declared in launch.h.
#include "launch.h"

using namespace esmi;
ESMI_TU_RANGE_SETTER(convgemm_bf16)

namespace esmi {

int launch_convgemm_stream_bf16(const ConvGemmP& p, int nt, dim3 grid, hipStream_t st) {
    const dim3 block(256);
    switch (nt) {
        case 1: ESMI_LAUNCH((convgemm_bf16_kernel<1>), grid, block, 0, st, p); break;
        case 2: ESMI_LAUNCH((convgemm_bf16_kernel<2>), grid, block, 0, st, p); break;
        case 4: ESMI_LAUNCH((convgemm_bf16_kernel<4>), grid, block, 0, st, p); break;
        case 8: ESMI_LAUNCH((convgemm_bf16_kernel<8>), grid, block, 0, st, p); break;
        default: return ESMI_ERR_UNSUPPORTED;
    }
    return launch_status();
}

int launch_convgemm_len_bf16(const ConvGemmP& p, int nt, dim3 grid, hipStream_t st) {
    const dim3 block(256);
    if (nt == 1) { ESMI_LAUNCH((convgemm_bf16_len_kernel<1>), grid, block, 0, st, p); }
    else if (nt == 2) { ESMI_LAUNCH((convgemm_bf16_len_kernel<2>), grid, block, 0, st, p); }
    else return ESMI_ERR_UNSUPPORTED;
    return launch_status();
}

#if ESMI_CHAIN_SPLIT
int launch_pwgemm_bf16(const ConvGemmP& p, bool full_row, dim3 grid, int n_items, hipStream_t st) {
#define ESMI_PW_BF16_CASE(KS_, NT_) ESMI_LAUNCH_LDS((pwgemm_bf16_kernel<KS_, NT_>), grid, dim3(64 * kPwWaves), pwgemm_lds_bytes<KS_>(), st, p, n_items)
    switch ((p.c_in == 128 ? 0 : 2) + (full_row ? 1 : 0)) {
        case 0: ESMI_PW_BF16_CASE(8, 2); break;
        case 1: ESMI_PW_BF16_CASE(8, 4); break;
        case 2: ESMI_PW_BF16_CASE(5, 2); break;
        default: ESMI_PW_BF16_CASE(5, 4); break;
    }
#undef ESMI_PW_BF16_CASE
    return launch_status();
}

int launch_convgemm_dma_bf16(const ConvGemmP& p, bool wide, int mt, dim3 grid, int lds_bytes, int nx, int ny, hipStream_t st) {
    constexpr int NWV = kGemmLdsWaves;
#define ESMI_DMA_BF16_CASE(NT_, MT_) ESMI_LAUNCH_LDS((convgemm_dma_bf16_kernel<NT_, MT_, NWV>), grid, dim3(64 * NWV), lds_bytes, st, p, nx, ny)
    if (wide) ESMI_DMA_BF16_CASE(8, 1);
    else if (mt == 2) ESMI_DMA_BF16_CASE(4, 2);
    else ESMI_DMA_BF16_CASE(4, 1);
#undef ESMI_DMA_BF16_CASE
    return launch_status();
}
#endif

}  // namespace esmi
