/* y4m.h — the YUV4MPEG2 container as a stream (libc only): a header line "YUV4MPEG2" + the tags W H F I A C X... in
 * any order, then per frame a line "FRAME[ params]" and the payload (the planes of struct nlk_yuv_format, include/
 * nlk_hip.h). Every malformed input is an error return with a one-line message in `err`: nothing aborts, nothing is
 * read or written past a buffer. Reads loop until their count is satisfied (pipes return short reads). */
#ifndef NLK_Y4M_H
#define NLK_Y4M_H

#include <stddef.h>
#include <stdio.h>

#include "nlk_hip.h"

#define Y4M_LINE_MAX 256 /* longest header or FRAME line, newline included */
#define Y4M_ERR_MAX 200 /* bytes of every `err` buffer */

struct y4m_header {
  int w, h;
  int fps_n, fps_d;   /* F (0:0 when absent) */
  int asp_n, asp_d;   /* A (0:0 when absent) */
  char interlace;     /* I: 'p' or '?' ('?' when absent); interlaced streams are refused */
  char ctag[32];      /* C as written, "" when absent */
  int range;          /* XCOLORRANGE: 1 = FULL, 0 = LIMITED, -1 = absent */
  struct nlk_yuv_format fmt; /* of C; full_range = (range == 1), matrix = 709: the caller overrides both */
  size_t frame_bytes; /* payload of one frame */
  char line[Y4M_LINE_MAX + 1]; /* the header line as read, newline included: the writer emits it verbatim */
  size_t line_len;
};

/* 0, or -1 with a message */
int y4m_read_header(FILE *f, struct y4m_header *hd, char *err);
/* 1: a frame was read into payload[frame_bytes]; 0: the stream ended before a FRAME line; -1 with a message: FRAME
 * misspelt, the line too long, the payload cut short, a read error */
int y4m_read_frame(FILE *f, const struct y4m_header *hd, void *payload, char *err);
/* 0, or -1 with a message */
int y4m_write_header(FILE *f, const struct y4m_header *hd, char *err);
int y4m_write_frame(FILE *f, const struct y4m_header *hd, const void *payload, char *err);

#endif
