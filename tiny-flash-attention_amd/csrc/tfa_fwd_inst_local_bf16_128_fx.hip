// one local (sliding-window) instantiation unit: dtype=bf16 head_dim=128 fixed-length
#define TFA_T __bf16
#define TFA_D 128
#define TFA_VARLEN false
#include "tfa_fwd_local_inst.inc"
