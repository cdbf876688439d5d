// tfa_kvc_inst_bf16_128.hip — the KV-cache form of the LDS-DMA kernel (tfa_fwd_kvcache), bf16, 128 wide.
#define TFA_T __bf16
#define TFA_D 128
#include "tfa_kvc_inst.inc"
