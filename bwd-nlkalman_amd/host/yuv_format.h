/* yuv_format.h — the two host-only functions of struct nlk_yuv_format (include/nlk_hip.h), stated once: libnlk_hip.so
 * exports them as nlk_yuv_format_from_tag / nlk_yuv_frame_bytes (csrc/tu_yuv.hip), and the container module
 * (host/y4m.c) uses them without linking anything but libc. */
#ifndef NLK_YUV_FORMAT_H
#define NLK_YUV_FORMAT_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "nlk_hip.h"

/* "" or a depth suffix "9".."16" (with `want_p`: a 'p' in front of it, as in 420p10); 0 if neither */
static inline int nlk_yuv_depth_suffix_(const char *s, int want_p, int *depth) {
  *depth = 8;
  if (!*s) return 1;
  if (want_p) {
    if (*s != 'p') return 0;
    ++s;
  }
  int d = 0, n = 0;
  if (*s == '0') return 0; /* (no leading zero: 420p010 is no tag) */
  for (; *s >= '0' && *s <= '9' && n < 2; ++s, ++n) d = d * 10 + (*s - '0');
  if (*s || n == 0 || d < 9 || d > 16) return 0;
  *depth = d;
  return 1;
}

/* 0, or NLK_EUNSUP for a tag the kernels do not cover (f is then left as it was) */
static inline int nlk_yuv_format_parse_(struct nlk_yuv_format *f, const char *tag) {
  struct nlk_yuv_format r = {0, 2, 2, 0, 8, 0, 709};
  if (!tag || !*tag || !strcmp(tag, "420jpeg")) {
    /* 4:2:0, chroma centred between the luma columns */
  } else if (!strcmp(tag, "420mpeg2")) {
    r.cosited_x = 1;
  } else if (!strncmp(tag, "420", 3) && nlk_yuv_depth_suffix_(tag + 3, 1, &r.depth)) {
    r.cosited_x = 1;
  } else if (!strncmp(tag, "422", 3) && nlk_yuv_depth_suffix_(tag + 3, 1, &r.depth)) {
    r.sy = 1;
    r.cosited_x = 1;
  } else if (!strncmp(tag, "444", 3) && nlk_yuv_depth_suffix_(tag + 3, 1, &r.depth)) {
    r.sx = r.sy = 1;
  } else if (!strncmp(tag, "mono", 4) && nlk_yuv_depth_suffix_(tag + 4, 0, &r.depth)) {
    r.mono = 1;
    r.sx = r.sy = 1;
  } else {
    return NLK_EUNSUP;
  }
  *f = r;
  return 0;
}

/* every field inside the ranges of include/nlk_hip.h */
static inline int nlk_yuv_format_ok_(const struct nlk_yuv_format *f) {
  if (!f || f->depth < 8 || f->depth > 16) return 0;
  if (f->full_range != 0 && f->full_range != 1) return 0;
  if (f->mono != 0 && f->mono != 1) return 0;
  if (f->mono) return 1;
  if ((f->sx != 1 && f->sx != 2) || (f->sy != 1 && f->sy != 2)) return 0;
  if (f->cosited_x != 0 && f->cosited_x != 1) return 0;
  return f->matrix == 601 || f->matrix == 709;
}

/* bytes of a frame; 0 if refused (a size < 1, a field out of range, more than SIZE_MAX / 2 bytes) */
static inline size_t nlk_yuv_frame_size_(int w, int h, const struct nlk_yuv_format *f) {
  if (w < 1 || h < 1 || !nlk_yuv_format_ok_(f)) return 0;
  const uint64_t bps = f->depth > 8 ? 2 : 1;
  uint64_t n = (uint64_t)w * (uint64_t)h; /* < 2^62 */
  if (!f->mono) {
    const uint64_t cw = ((uint64_t)w + f->sx - 1) / f->sx, chh = ((uint64_t)h + f->sy - 1) / f->sy;
    n += 2 * cw * chh;
  }
  if (n > (uint64_t)(SIZE_MAX / 2) / bps) return 0; /* (n < 3 * 2^62: the sum above cannot wrap) */
  return (size_t)(n * bps);
}

#endif /* NLK_YUV_FORMAT_H */
