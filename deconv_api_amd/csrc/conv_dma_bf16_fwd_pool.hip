// Instantiation unit of the LDS-DMA conv (conv_dma_impl.h): dma_run<DT_BF16, CONV_A_FWD, CONV_E_POOL>.
#include "conv_dma_impl.h"

int dv::dma_run_bf16_fwd_pool(const ConvArgs& a, const DmaPlan& p, hipStream_t s) {
  return dma_run<DT_BF16, CONV_A_FWD, CONV_E_POOL>(a, p, s);
}
