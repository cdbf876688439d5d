// tfa_kvc_inst_bf16_64.hip — the KV-cache form of the LDS-DMA kernel (tfa_fwd_kvcache), bf16, 64 wide.
#define TFA_T __bf16
#define TFA_D 64
#include "tfa_kvc_inst.inc"
