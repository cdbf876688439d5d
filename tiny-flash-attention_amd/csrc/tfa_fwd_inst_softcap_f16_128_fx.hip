// one soft-capping (softcap) instantiation unit: dtype=f16 head_dim=128 fixed-length
#define TFA_T _Float16
#define TFA_D 128
#define TFA_VARLEN false
#define TFA_LOCAL true
#define TFA_CAUSAL true
#define TFA_SOFTCAP true
#include "tfa_fwd_form_inst.inc"
