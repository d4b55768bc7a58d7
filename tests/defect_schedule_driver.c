/* defect_schedule_driver.c — nlk_defect_schedule (bwd-nlkalman_amd/host/defect_schedule.c) as a stand-alone program for
 * tests/test_defect_map.py: "defect_schedule_driver K_SIGMA T_LAST N..." prints, for every N and t = 1 .. T_LAST, one
 * line "N t THR GAIN code" with the two floats as their bits in hexadecimal; then the refused calls, "refused code".
 * Links defect_schedule.c alone. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "nlk_hip.h"

static unsigned bits(float f) {
  uint32_t u;
  memcpy(&u, &f, sizeof u);
  return u;
}

int main(int argc, char **argv) {
  if (argc < 4) return 2;
  const float k_sigma = strtof(argv[1], NULL);
  const long last = strtol(argv[2], NULL, 10);
  for (int i = 3; i < argc; ++i) {
    const int n = atoi(argv[i]);
    for (long t = 1; t <= last; ++t) {
      float thr = -1.f, gain = -1.f;
      const int code = nlk_defect_schedule(t, n, k_sigma, &thr, &gain);
      printf("%d %ld %08x %08x %d\n", n, t, bits(thr), bits(gain), code);
    }
  }
  float thr = -1.f, gain = -1.f;
  printf("refused %d %d %d %d\n", nlk_defect_schedule(0, 32, k_sigma, &thr, &gain),
         nlk_defect_schedule(1, 0, k_sigma, &thr, &gain), nlk_defect_schedule(1, 32, k_sigma, NULL, &gain),
         nlk_defect_schedule(1, 32, k_sigma, &thr, NULL));
  printf("untouched %d\n", thr == -1.f && gain == -1.f);
  return 0;
}
