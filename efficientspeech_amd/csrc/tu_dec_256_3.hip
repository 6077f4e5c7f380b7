// esmi C-ABI, translation unit "tu_dec_256_3.hip": mel_decoder_kernel<256, 3, NW> and its launcher (mel_decoder.h, ESMI_DEC_INSTANCE)
#include "launch.h"
#include "mel_decoder.h"

ESMI_DEC_INSTANCE(256, 3, PM_SPLIT)
