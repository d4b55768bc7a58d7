/* y4m_driver.c — a stand-alone program around host/y4m.c for tests/test_y4m.py (built there with
 * -fsanitize=address,undefined where the compiler can): reads the stream named by argv[1] to its end, writes every
 * frame to a scratch file, prints "ok W H frames N" (exit 0) or "error: <message>" (exit 1). */
#include <stdio.h>
#include <stdlib.h>

#include "y4m.h"

int main(int argc, char **argv) {
  char err[Y4M_ERR_MAX];
  struct y4m_header hd;
  FILE *in = argc > 1 ? fopen(argv[1], "rb") : NULL, *out = tmpfile();
  if (!in || !out) { printf("error: cannot open the files\n"); return 1; }
  if (y4m_read_header(in, &hd, err)) { printf("error: %s\n", err); return 1; }
  void *buf = malloc(hd.frame_bytes);
  if (!buf || y4m_write_header(out, &hd, err)) { printf("error: setup\n"); return 1; }
  long n = 0;
  int r;
  while ((r = y4m_read_frame(in, &hd, buf, err)) == 1) {
    if (y4m_write_frame(out, &hd, buf, err)) { printf("error: %s\n", err); return 1; }
    ++n;
  }
  free(buf);
  fclose(in);
  fclose(out);
  if (r < 0) { printf("error: frame %ld: %s\n", n + 1, err); return 1; }
  printf("ok %d %d frames %ld\n", hd.w, hd.h, n);
  return 0;
}
