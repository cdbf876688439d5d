// one packed variable-length backward instantiation unit: dtype=bf16 head_dim=128
#define TFA_T __bf16
#define TFA_D 128
#include "tfa_bwd_varlen_inst.inc"
