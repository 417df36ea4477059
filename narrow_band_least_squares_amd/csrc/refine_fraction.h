// The three-point parabola vertex shared by the lag refinement (refine.hip) and the peak offsets of the Capon / Bartlett
// spectra (capon.hip): for the values rm, r0, rp at the positions -1, 0, +1 the vertex lies at
//   frac = 0.5 (rm - rp) / ((rm - 2 r0) + rp),   clamped to [-1/2, 1/2]
// and is 0 unless all three values are finite, the denominator is < 0 (a strict maximum) and the quotient is finite;
// -0.0 becomes 0.0.  Both translation units are built without contraction (2 r0 is exact either way).
#pragma once
#include "wave_ops.h"

__device__ inline double refine_fraction(double rm, double r0, double rp) {
    const double nn = rm - rp;
    const double dd = (rm - 2.0 * r0) + rp;
    double f = 0.5 * nn / dd;
    const bool ok = nbls_wave::finite_f64(rm) && nbls_wave::finite_f64(r0) && nbls_wave::finite_f64(rp) && dd < 0.0 &&
                    nbls_wave::finite_f64(f);
    if (!ok || f == 0.0) return 0.0;          // (also turns -0.0 into 0.0)
    return f < -0.5 ? -0.5 : (f > 0.5 ? 0.5 : f);
}
