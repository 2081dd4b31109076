// What the conjugate-gradient driver (csrc/pcg.hip: nksr_pcg_run) calls of the coarse-level block preconditioner (csrc/cheb.hip).
// Internal to the library: the symbols stay out of its dynamic table.
#pragma once
#include "pcg_dev.h"

#pragma GCC visibility push(hidden)
// NKSR_OK, or the error set for a block that cannot be applied (pc->n <= 0, steps, interval, NULL arrays)
int cheb_check(const nksr_coarse_precond_t* pc, int nseg);
// pc->coef <- every segment's polynomial for its interval (pc->lambda, pc->gersh, pc->lambda_scale, pc->ratio, pc->steps)
void cheb_coeffs(const nksr_coarse_precond_t* pc, int nseg, hipStream_t st);
// z_c = p_k(A_cc) r_c  (r, z: the coarse slices of the PCG vectors); sc (may be NULL): segments that are done or on Jacobi are left alone
void cheb_apply(const nksr_coarse_precond_t* pc, const float* r, float* z, const SegScalars* sc, hipStream_t st);
#pragma GCC visibility pop
