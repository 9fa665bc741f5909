// The entry points of the other conv translation units that conv.hip's
// dispatchers call.
#pragma once

#include "common.h"

// conv_fp32.hip: fp32 kernel path
at::Tensor conv2d_fwd_into_fp32(at::Tensor x, at::Tensor w, at::Tensor y,
                                int64_t Ho, int64_t Wo, int64_t sh, int64_t sw,
                                int64_t ph, int64_t pw, int64_t dh, int64_t dw,
                                int64_t groups, int64_t osh, int64_t osw,
                                int64_t oh0, int64_t ow0,
                                at::Tensor* part_out);

// conv2.hip: the v2 ring. _v2p pads the weight span itself, _v2_flat takes
// it span-padded already, _v2_into scatters into the caller's canvas.
at::Tensor conv2d_fwd_v2p(at::Tensor x, at::Tensor w, int64_t sh, int64_t sw,
                          int64_t ph, int64_t pw, int64_t dh, int64_t dw,
                          int64_t groups, at::Tensor* part_out);
at::Tensor conv2d_fwd_v2_flat(at::Tensor x, at::Tensor wp, int64_t Kt_,
                              int64_t Cg_, int64_t R_, int64_t S_, int64_t sh,
                              int64_t sw, int64_t ph, int64_t pw, int64_t dh,
                              int64_t dw, int64_t groups,
                              at::Tensor* part_out,
                              at::Tensor* acc_into = nullptr);
at::Tensor conv2d_fwd_v2_into(at::Tensor x, at::Tensor w, at::Tensor y,
                              int64_t Ho, int64_t Wo, int64_t groups,
                              int64_t osh, int64_t osw, int64_t oh0,
                              int64_t ow0, bool acc = false);

// conv_halo.hip: halo-staged 3x3 / stride 1 / pad 1 / 64->64 kernel
bool conv3x3_halo_admits(int64_t N, int64_t H, int64_t W);
void conv3x3_halo_launch(const at::Tensor& x, const at::Tensor& w,
                         at::Tensor& y, const at::Tensor& zbuf, float* part);
