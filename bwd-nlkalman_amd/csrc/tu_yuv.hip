// tu_yuv.hip — planar Y'CbCr frames <-> HWC float RGB: the entry points of include/nlk_hip.h (kernels: k_yuv.h; the
// two host-only functions of the format: host/yuv_format.h)
#include "k_yuv.h"
#include "nlk_internal.h"

#include "../host/yuv_format.h"

namespace {

// the constants of DESIGN.md §9, in double, rounded to float once
NlkYuvK yuv_constants(const nlk_yuv_format& f) {
  const double s = (double)(1 << (f.depth - 8)), top = (double)((1 << f.depth) - 1);
  const double y0 = f.full_range ? 0.0 : 16.0 * s, c0 = 128.0 * s;
  const double ky = f.full_range ? 255.0 / top : 255.0 / (219.0 * s);
  const double kc = f.full_range ? 255.0 / top : 255.0 / (224.0 * s);
  const double kr = f.matrix == 601 ? 0.299 : 0.2126, kb = f.matrix == 601 ? 0.114 : 0.0722;
  const double kg = 1.0 - kr - kb;
  const double crr = 2.0 * (1.0 - kr), cbu = 2.0 * (1.0 - kb);
  const double cgu = 2.0 * kb * (1.0 - kb) / kg, cgv = 2.0 * kr * (1.0 - kr) / kg;
  NlkYuvK k;
  k.y0 = (float)y0; k.ky = (float)ky; k.c0 = (float)c0; k.kc = (float)kc;
  k.crr = (float)crr; k.cbu = (float)cbu; k.cgu = (float)cgu; k.cgv = (float)cgv;
  k.kr = (float)kr; k.kg = (float)kg; k.kb = (float)kb;
  k.icbu = (float)(1.0 / cbu); k.icrr = (float)(1.0 / crr); k.iky = (float)(1.0 / ky); k.ikc = (float)(1.0 / kc);
  k.maxc = (float)top;
  return k;
}

template <bool TO_RGB, typename T, int SX, int SY, bool COS, bool MONO>
void yuv_launch(nlk_ctx* c, dim3 grid, float* rgb, void* yuv, int w, int h, const NlkYuvK& k) {
  const dim3 block(NLK_YUV_BX, NLK_YUV_BY);
  if (TO_RGB)
    hipLaunchKernelGGL((k_yuv_to_rgb<T, SX, SY, COS, MONO>), grid, block, 0, c->stream, rgb, (const T*)yuv, w, h, k);
  else
    hipLaunchKernelGGL((k_rgb_to_yuv<T, SX, SY, COS, MONO>), grid, block, 0, c->stream, (T*)yuv, (const float*)rgb, w, h, k);
}

// the instantiation of a format: sample width, subsampling per axis, siting (which only a subsampled axis has), mono
template <bool TO_RGB, typename T>
void yuv_dispatch(nlk_ctx* c, dim3 grid, float* rgb, void* yuv, int w, int h, const nlk_yuv_format& f, const NlkYuvK& k) {
  if (f.mono) return yuv_launch<TO_RGB, T, 1, 1, false, true>(c, grid, rgb, yuv, w, h, k);
  if (f.sx == 1) {
    if (f.sy == 1) return yuv_launch<TO_RGB, T, 1, 1, false, false>(c, grid, rgb, yuv, w, h, k);
    return yuv_launch<TO_RGB, T, 1, 2, false, false>(c, grid, rgb, yuv, w, h, k);
  }
  if (f.sy == 1) {
    if (f.cosited_x) return yuv_launch<TO_RGB, T, 2, 1, true, false>(c, grid, rgb, yuv, w, h, k);
    return yuv_launch<TO_RGB, T, 2, 1, false, false>(c, grid, rgb, yuv, w, h, k);
  }
  if (f.cosited_x) return yuv_launch<TO_RGB, T, 2, 2, true, false>(c, grid, rgb, yuv, w, h, k);
  return yuv_launch<TO_RGB, T, 2, 2, false, false>(c, grid, rgb, yuv, w, h, k);
}

template <bool TO_RGB>
int yuv_run(nlk_ctx* c, const char* who, float* rgb, void* yuv, int w, int h, const nlk_yuv_format* f) {
  if (!c || !rgb || !yuv || !f) return fail(c, NLK_EINVAL, "%s: NULL argument", who);
  if (w < 1 || h < 1) return fail(c, NLK_EINVAL, "%s: size %d x %d", who, w, h);
  if (!nlk_yuv_format_ok_(f))
    return fail(c, NLK_EINVAL,
                "%s: format {mono %d, sx %d, sy %d, cosited_x %d, depth %d, full_range %d, matrix %d} is out of range", who,
                f->mono, f->sx, f->sy, f->cosited_x, f->depth, f->full_range, f->matrix);
  const unsigned gx = ((unsigned)(w + 3) / 4 + NLK_YUV_BX - 1) / NLK_YUV_BX, gy = ((unsigned)(h + 1) / 2 + NLK_YUV_BY - 1) / NLK_YUV_BY;
  if (gy > 65535u) return fail(c, NLK_EUNSUP, "%s: %d rows are more than one launch covers", who, h);
  NLK_USE_DEVICE(c);
  const NlkYuvK k = yuv_constants(*f);
  if (f->depth > 8)
    yuv_dispatch<TO_RGB, uint16_t>(c, dim3(gx, gy), rgb, yuv, w, h, *f, k);
  else
    yuv_dispatch<TO_RGB, uint8_t>(c, dim3(gx, gy), rgb, yuv, w, h, *f, k);
  HIPCHK(c, hipGetLastError());
  return NLK_OK;
}

}  // namespace

extern "C" {

int nlk_yuv_format_from_tag(struct nlk_yuv_format* f, const char* ctag) {
  if (!f) return fail(nullptr, NLK_EINVAL, "nlk_yuv_format_from_tag: NULL argument");
  if (nlk_yuv_format_parse_(f, ctag) != 0)
    return fail(nullptr, NLK_EUNSUP, "nlk_yuv_format_from_tag: colour space \"%s\" is not supported", ctag);
  return NLK_OK;
}

size_t nlk_yuv_frame_bytes(int w, int h, const struct nlk_yuv_format* f) { return nlk_yuv_frame_size_(w, h, f); }

int nlk_dev_yuv_to_rgb(nlk_ctx* c, float* d_rgb, const void* d_yuv, int w, int h, const struct nlk_yuv_format* f) {
  return yuv_run<true>(c, "nlk_dev_yuv_to_rgb", d_rgb, const_cast<void*>(d_yuv), w, h, f);
}

int nlk_dev_rgb_to_yuv(nlk_ctx* c, void* d_yuv, const float* d_rgb, int w, int h, const struct nlk_yuv_format* f) {
  return yuv_run<false>(c, "nlk_dev_rgb_to_yuv", const_cast<float*>(d_rgb), d_yuv, w, h, f);
}

}  // extern "C"
