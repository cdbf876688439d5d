// one soft-capping (softcap) backward instantiation unit: dtype=f16 head_dim=128 fixed-length
#define TFA_T _Float16
#define TFA_D 128
#define TFA_VARLEN false
#define TFA_LOCAL true
#define TFA_SOFTCAP true
#include "tfa_bwd_form_inst.inc"
