// esmi C-ABI, translation unit "tu_dec_128_5.hip": mel_decoder_kernel<128, 5, NW> and its launcher (mel_decoder.h, ESMI_DEC_INSTANCE)
#include "launch.h"
#include "mel_decoder.h"

ESMI_DEC_INSTANCE(128, 5, PM_SPLIT)
