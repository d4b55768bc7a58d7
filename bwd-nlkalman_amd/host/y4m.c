/* y4m.c — see y4m.h */
#include "y4m.h"

#include <errno.h>
#include <limits.h>
#include <stdarg.h>
#include <string.h>

#include "yuv_format.h"

static int bad(char *err, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(err, Y4M_ERR_MAX, fmt, ap);
  va_end(ap);
  return -1;
}

/* a line of at most Y4M_LINE_MAX bytes, newline included, into line[Y4M_LINE_MAX + 1] (terminated). Returns its
 * length, 0 at the end of the stream before any byte, -1 when it has no newline within the limit, -2 when the stream
 * ends inside it */
static int read_line(FILE *f, char *line) {
  int n = 0;
  for (;;) {
    const int c = fgetc(f);
    if (c == EOF) {
      line[n] = 0;
      return n == 0 ? 0 : -2;
    }
    line[n++] = (char)c;
    if (c == '\n') break;
    if (n == Y4M_LINE_MAX) {
      line[n] = 0;
      return -1;
    }
  }
  line[n] = 0;
  return n;
}

/* decimal digits only, 0 .. INT_MAX; -1 otherwise. *end = the first byte after them */
static long number(const char *s, const char **end) {
  long v = 0;
  const char *p = s;
  for (; *p >= '0' && *p <= '9'; ++p) {
    v = v * 10 + (*p - '0');
    if (v > INT_MAX) return -1;
  }
  *end = p;
  return p == s ? -1 : v;
}

static int ratio(const char *s, int *n, int *d) {
  const char *e;
  const long a = number(s, &e);
  if (a < 0 || *e != ':') return -1;
  const long b = number(e + 1, &e);
  if (b < 0 || *e) return -1;
  *n = (int)a;
  *d = (int)b;
  return 0;
}

int y4m_read_header(FILE *f, struct y4m_header *hd, char *err) {
  memset(hd, 0, sizeof *hd);
  hd->interlace = '?';
  hd->range = -1;
  const int n = read_line(f, hd->line);
  if (n == 0) return bad(err, "empty stream: no YUV4MPEG2 header");
  if (n == -1) return bad(err, "the header line is longer than %d bytes", Y4M_LINE_MAX);
  if (n == -2) return bad(err, "the stream ends inside the header line");
  hd->line_len = (size_t)n;
  if (memchr(hd->line, 0, (size_t)n)) return bad(err, "the header line holds a NUL byte");
  if (strncmp(hd->line, "YUV4MPEG2", 9) || (hd->line[9] != ' ' && hd->line[9] != '\n'))
    return bad(err, "not a YUV4MPEG2 stream (the magic is missing)");
  char copy[Y4M_LINE_MAX + 1];
  memcpy(copy, hd->line + 9, (size_t)n - 9 + 1);
  copy[n - 9 - 1] = 0; /* (the newline) */
  int have_w = 0, have_h = 0;
  for (char *tok = strtok(copy, " "); tok; tok = strtok(NULL, " ")) {
    const char *v = tok + 1, *e;
    switch (tok[0]) {
      case 'W':
      case 'H': {
        const long x = number(v, &e);
        if (x < 1 || *e) return bad(err, "header: %c%s is not a positive size", tok[0], v);
        if (tok[0] == 'W') { hd->w = (int)x; have_w = 1; } else { hd->h = (int)x; have_h = 1; }
        break;
      }
      case 'F':
        if (ratio(v, &hd->fps_n, &hd->fps_d)) return bad(err, "header: F%s is not a frame rate N:D", v);
        break;
      case 'A':
        if (ratio(v, &hd->asp_n, &hd->asp_d)) return bad(err, "header: A%s is not an aspect ratio N:D", v);
        break;
      case 'I':
        if ((v[0] != 'p' && v[0] != '?') || v[1]) return bad(err, "header: I%s: interlaced streams are not supported", v);
        hd->interlace = v[0];
        break;
      case 'C':
        if (strlen(v) >= sizeof hd->ctag || nlk_yuv_format_parse_(&hd->fmt, v))
          return bad(err, "header: colour space C%s is not supported", v);
        strcpy(hd->ctag, v);
        break;
      case 'X':
        if (!strcmp(v, "COLORRANGE=FULL")) hd->range = 1;
        else if (!strcmp(v, "COLORRANGE=LIMITED")) hd->range = 0;
        break; /* (every other X tag is kept: the header line is written as read) */
      default:
        break; /* unknown tags are kept too */
    }
  }
  if (!have_w || !have_h) return bad(err, "header: %s is missing", have_w ? "H" : "W");
  if (!hd->ctag[0]) nlk_yuv_format_parse_(&hd->fmt, NULL);
  hd->fmt.full_range = hd->range == 1;
  hd->frame_bytes = nlk_yuv_frame_size_(hd->w, hd->h, &hd->fmt);
  if (!hd->frame_bytes) return bad(err, "header: a %d x %d frame is too large", hd->w, hd->h);
  return 0;
}

int y4m_read_frame(FILE *f, const struct y4m_header *hd, void *payload, char *err) {
  char line[Y4M_LINE_MAX + 1];
  const int n = read_line(f, line);
  if (n == 0) return 0;
  if (n == -1) return bad(err, "a FRAME line is longer than %d bytes", Y4M_LINE_MAX);
  if (n == -2 || strncmp(line, "FRAME", 5) || (line[5] != ' ' && line[5] != '\n'))
    return bad(err, n == -2 ? "the stream ends inside a FRAME line" : "FRAME expected");
  size_t got = 0;
  while (got < hd->frame_bytes) {
    const size_t r = fread((char *)payload + got, 1, hd->frame_bytes - got, f);
    if (r == 0) {
      if (ferror(f) && errno == EINTR) { clearerr(f); continue; }
      if (ferror(f)) return bad(err, "read error: %s", strerror(errno));
      return bad(err, "the stream ends inside a frame (%zu of %zu bytes)", got, hd->frame_bytes);
    }
    got += r;
  }
  return 1;
}

static int put(FILE *f, const void *p, size_t n, char *err) {
  if (fwrite(p, 1, n, f) != n) return bad(err, "write error: %s", strerror(errno));
  return 0;
}

int y4m_write_header(FILE *f, const struct y4m_header *hd, char *err) { return put(f, hd->line, hd->line_len, err); }

int y4m_write_frame(FILE *f, const struct y4m_header *hd, const void *payload, char *err) {
  if (put(f, "FRAME\n", 6, err) || put(f, payload, hd->frame_bytes, err)) return -1;
  return 0;
}
