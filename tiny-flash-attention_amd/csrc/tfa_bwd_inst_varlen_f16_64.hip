// one packed variable-length backward instantiation unit: dtype=f16 head_dim=64
#define TFA_T _Float16
#define TFA_D 64
#define TFA_VARLEN true
#define TFA_LOCAL false
#include "tfa_bwd_form_inst.inc"
