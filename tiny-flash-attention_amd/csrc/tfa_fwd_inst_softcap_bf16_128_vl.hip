// one soft-capping (softcap) instantiation unit: dtype=bf16 head_dim=128 packed variable-length
#define TFA_T __bf16
#define TFA_D 128
#define TFA_VARLEN true
#define TFA_LOCAL true
#define TFA_CAUSAL true
#define TFA_SOFTCAP true
#include "tfa_fwd_form_inst.inc"
