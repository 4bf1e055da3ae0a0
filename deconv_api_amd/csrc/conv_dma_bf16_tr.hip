// Instantiation unit of the LDS-DMA conv (conv_dma_impl.h): dma_run<DT_BF16, CONV_A_TRANSPOSE, CONV_E_BF16>.
#include "conv_dma_impl.h"

int dv::dma_run_bf16_tr(const ConvArgs& a, const DmaPlan& p, hipStream_t s) {
  return dma_run<DT_BF16, CONV_A_TRANSPOSE, CONV_E_BF16>(a, p, s);
}
