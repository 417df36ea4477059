// The beam at the solved slowness steered at fractional-sample delays (nbls_set_beam_interpolation): the
// TAPS = 4, 6 and 8 instances of beam_fstat_kernel, plain and KEPT, and their launch — beam.hip built a second time, so
// that beam.o holds the two whole-sample instances and nothing else, as it did.
#define NBLS_BEAM_STEER 1
#include "beam.hip"
