// tfa_kvc8_inst_f16_64.hip — the e4m3 (fp8 K/V cache) form of the KV-cache kernel (tfa_fwd_kvcache_fp8), q / out f16, 64 wide.
#define TFA_T _Float16
#define TFA_D 64
#include "tfa_kvc8_inst.inc"
