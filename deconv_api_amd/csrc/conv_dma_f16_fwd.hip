// Instantiation unit of the LDS-DMA conv (conv_dma_impl.h): dma_run<DT_F16, CONV_A_FWD, CONV_E_BF16>.
#include "conv_dma_impl.h"

int dv::dma_run_f16_fwd(const ConvArgs& a, const DmaPlan& p, hipStream_t s) {
  return dma_run<DT_F16, CONV_A_FWD, CONV_E_BF16>(a, p, s);
}
