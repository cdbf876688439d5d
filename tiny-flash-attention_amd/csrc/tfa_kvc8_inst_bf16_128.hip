// tfa_kvc8_inst_bf16_128.hip — the e4m3 (fp8 K/V cache) form of the KV-cache kernel (tfa_fwd_kvcache_fp8), q / out bf16, 128 wide.
#define TFA_T __bf16
#define TFA_D 128
#include "tfa_kvc8_inst.inc"
