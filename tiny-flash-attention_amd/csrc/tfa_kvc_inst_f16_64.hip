// tfa_kvc_inst_f16_64.hip — the KV-cache form of the LDS-DMA kernel (tfa_fwd_kvcache), f16, 64 wide.
#define TFA_T _Float16
#define TFA_D 64
#include "tfa_kvc_inst.inc"
