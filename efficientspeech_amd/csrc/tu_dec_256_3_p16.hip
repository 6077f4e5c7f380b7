// esmi C-ABI, translation unit "tu_dec_256_3_p16.hip": mel_decoder_kernel<256, 3, NW, true>, the precision-16 form (include/esmi.h), and its launcher (mel_decoder.h, ESMI_DEC_INSTANCE)
#include "launch.h"
#include "mel_decoder.h"

ESMI_DEC_INSTANCE(256, 3, PM_F16)
