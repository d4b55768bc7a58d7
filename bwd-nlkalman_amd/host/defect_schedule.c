/* defect_schedule.c — nlk_defect_schedule (include/nlk_hip.h): the threshold and the gain of nlk_dev_defect_step for
 * the frame of index t, stated once for the C tools (host/seq_step.c, host/main_defects.c), sequence.py and the tests
 * (tests/defectmap_ref.py restates it in numpy). Host only, plain C: nothing of the device libraries is needed to link
 * it (libnlk_hip.so links it in and exports it). */
#include <math.h>

#include "nlk_hip.h"

int nlk_defect_schedule(long t, int n_window, float k_sigma, float *thr, float *gain) {
  if (t < 1 || n_window < 1 || !thr || !gain) return NLK_EINVAL;
  const long n = n_window;
  /* an exact mean of the first N frames, then an exponential window: its noise is below sigma / sqrt(N) */
  *gain = 1.f / (float)(t + 1 < n ? t + 1 : n);
  *thr = k_sigma * sqrtf(1.f / (float)(t < n ? t : n));
  return NLK_OK;
}
