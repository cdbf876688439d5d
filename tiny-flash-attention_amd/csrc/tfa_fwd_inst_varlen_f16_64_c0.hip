// one packed variable-length instantiation unit: dtype=f16 head_dim=64 causal=0
#define TFA_T _Float16
#define TFA_D 64
#define TFA_CAUSAL false
#define TFA_VARLEN true
#define TFA_LOCAL false
#include "tfa_fwd_form_inst.inc"
