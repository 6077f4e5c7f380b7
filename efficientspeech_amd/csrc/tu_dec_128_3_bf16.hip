// esmi C-ABI, translation unit "tu_dec_128_3_bf16.hip": mel_decoder_bf16_kernel<128, 3, NW>, the bf16 form (include/esmi.h), and its launcher (mel_decoder.h, ESMI_DEC_INSTANCE)
#include "launch.h"
#include "mel_decoder.h"

ESMI_DEC_INSTANCE(128, 3, PM_BF16)
