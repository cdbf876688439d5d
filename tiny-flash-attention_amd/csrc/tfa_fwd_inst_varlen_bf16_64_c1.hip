// one packed variable-length instantiation unit: dtype=bf16 head_dim=64 causal=1
#define TFA_T __bf16
#define TFA_D 64
#define TFA_CAUSAL true
#define TFA_VARLEN true
#define TFA_LOCAL false
#include "tfa_fwd_form_inst.inc"
