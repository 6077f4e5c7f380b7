// esmi C-ABI, translation unit "tu_dec_256_5_bf16.hip": mel_decoder_bf16_kernel<256, 5, NW> -- the bf16 form (include/esmi.h) -- and its
// launcher (mel_decoder.h, ESMI_DEC_INSTANCE_BF16).  The exact-fp32 build has no one-product path: no kernel in this unit there.
#include "launch.h"
#include "dec_layout.h"

ESMI_TU_RANGE_SETTER(dec_256_5_bf16)
#if ESMI_DEC_SPLIT == 2
#include "mel_decoder.h"

ESMI_DEC_INSTANCE_BF16(256, 5)
#endif
