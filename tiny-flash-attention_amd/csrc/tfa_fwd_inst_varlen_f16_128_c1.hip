// one packed variable-length instantiation unit: dtype=f16 head_dim=128 causal=1
#define TFA_T _Float16
#define TFA_D 128
#define TFA_CAUSAL true
#define TFA_VARLEN true
#define TFA_LOCAL false
#include "tfa_fwd_form_inst.inc"
