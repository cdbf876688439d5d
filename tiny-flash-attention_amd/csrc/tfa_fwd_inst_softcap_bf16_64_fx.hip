// one soft-capping (softcap) instantiation unit: dtype=bf16 head_dim=64 fixed-length
#define TFA_T __bf16
#define TFA_D 64
#define TFA_VARLEN false
#define TFA_LOCAL true
#define TFA_CAUSAL true
#define TFA_SOFTCAP true
#include "tfa_fwd_form_inst.inc"
