// tfa_kvc8_inst_f16_128.hip — the e4m3 (fp8 K/V cache) form of the KV-cache kernel (tfa_fwd_kvcache_fp8), q / out f16, 128 wide.
#define TFA_T _Float16
#define TFA_D 128
#include "tfa_kvc8_inst.inc"
