// esmi C-ABI, translation unit "tu_hifigan_bf16.hip": the one-launch ResBlock kernels of the HiFi-GAN generator at bf16
// (hifigan_resblock.h: one bfloat16 product per contraction, ESMI_PRECISION_BF16).  A unit of its own: its twelve instantiations compile beside
// tu_hifigan.hip's instead of behind them (launch.h has the ladder they hang on; the exact-fp32 build has none of them).  The generator's
// host side (tu_hifigan.hip) decides when they run.
// One of several translation units of libesmi.so (compiled in parallel by __graft_entry__.build(); the simulator build
// tools/wavesim/build.sh compiles the same files with the host compiler).  Internal launchers are declared in launch.h.
#include "launch.h"

using namespace esmi;
ESMI_TU_RANGE_SETTER(hifigan_bf16)
ESMI_RESBLOCK_INSTANCE(PM_BF16)
