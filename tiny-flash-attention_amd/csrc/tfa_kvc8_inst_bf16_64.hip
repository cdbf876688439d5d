// tfa_kvc8_inst_bf16_64.hip — the e4m3 (fp8 K/V cache) form of the KV-cache kernel (tfa_fwd_kvcache_fp8), q / out bf16, 64 wide.
#define TFA_T __bf16
#define TFA_D 64
#include "tfa_kvc8_inst.inc"
