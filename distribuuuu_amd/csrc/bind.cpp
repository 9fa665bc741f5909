// Python bindings for the gfx950 kernel set.
#include <torch/extension.h>

// elementwise.hip
at::Tensor relu_fwd(at::Tensor x);
at::Tensor relu_bwd(at::Tensor gy, at::Tensor y);
at::Tensor add_relu_fwd(at::Tensor a, at::Tensor b);
at::Tensor se_scale_fwd(at::Tensor x, at::Tensor s);
at::Tensor dropout_fwd(at::Tensor x, double p, int64_t seed);
at::Tensor dropout_fwd_dev(at::Tensor x, double p, int64_t salt,
                           at::Tensor step_dev);
std::vector<at::Tensor> se_scale_bwd(at::Tensor gy, at::Tensor x,
                                     at::Tensor s);
// bn.hip
std::vector<at::Tensor> bn_sums(at::Tensor x);
at::Tensor bn_reduce_partials(at::Tensor part);
std::vector<at::Tensor> bn_stats(at::Tensor x, at::Tensor gamma,
                                 at::Tensor beta,
                                 c10::optional<at::Tensor> rm_opt,
                                 c10::optional<at::Tensor> rv_opt,
                                 double momentum, double eps, bool training,
                                 c10::optional<at::Tensor> part_opt);
at::Tensor bn_apply_act(at::Tensor x, at::Tensor scale, at::Tensor shift,
                        int64_t act, c10::optional<at::Tensor> res);
at::Tensor bn_bwd_stats(at::Tensor gy, at::Tensor x,
                        c10::optional<at::Tensor> res, at::Tensor scale,
                        at::Tensor shift, int64_t act);
std::vector<at::Tensor> bn_bwd_apply(at::Tensor gy, at::Tensor x,
                                     c10::optional<at::Tensor> res,
                                     at::Tensor mean, at::Tensor rstd,
                                     at::Tensor gamma, at::Tensor scale,
                                     at::Tensor shift, at::Tensor sums,
                                     double total_count, int64_t act,
                                     bool training, bool need_gres);
std::vector<at::Tensor> bn_bwd(at::Tensor gy, at::Tensor x,
                               c10::optional<at::Tensor> res, at::Tensor mean,
                               at::Tensor rstd, at::Tensor gamma,
                               at::Tensor scale, at::Tensor shift,
                               int64_t act, bool training, bool need_gres,
                               c10::optional<at::Tensor> mask);
std::vector<at::Tensor> bn_apply_act_mask(at::Tensor x, at::Tensor scale,
                                          at::Tensor shift, int64_t act,
                                          at::Tensor res,
                                          c10::optional<at::Tensor> res_scale,
                                          c10::optional<at::Tensor> res_shift);
std::vector<at::Tensor> bn_act_maxpool_fwd(at::Tensor x, at::Tensor scale,
                                           at::Tensor shift, int64_t act);
at::Tensor bn_pool_bwd_stats(at::Tensor gpool, at::Tensor idx, at::Tensor x,
                             at::Tensor scale, at::Tensor shift, int64_t act);
std::vector<at::Tensor> bn_pool_bwd_apply(at::Tensor gpool, at::Tensor idx,
                                          at::Tensor x, at::Tensor mean,
                                          at::Tensor rstd, at::Tensor gamma,
                                          at::Tensor scale, at::Tensor shift,
                                          at::Tensor sums, double total_count,
                                          int64_t act, bool training);
std::vector<at::Tensor> bn_pool_bwd(at::Tensor gpool, at::Tensor idx,
                                    at::Tensor x, at::Tensor mean,
                                    at::Tensor rstd, at::Tensor gamma,
                                    at::Tensor scale, at::Tensor shift,
                                    int64_t act, bool training);
// pool.hip
std::vector<at::Tensor> maxpool_fwd(at::Tensor x, int64_t K, int64_t S,
                                    int64_t P);
at::Tensor maxpool_bwd(at::Tensor gy, at::Tensor idx, int64_t H, int64_t W,
                       int64_t K, int64_t S, int64_t P);
at::Tensor gap_fwd(at::Tensor x);
at::Tensor gap_bwd(at::Tensor gy, int64_t H, int64_t W);
at::Tensor avgpool_fwd(at::Tensor x, int64_t K, int64_t S);
at::Tensor avgpool_bwd(at::Tensor gy, int64_t K, int64_t S, int64_t H,
                       int64_t W);
// loss.hip
std::vector<at::Tensor> ce_fwd(at::Tensor logits, at::Tensor target);
at::Tensor ce_bwd(at::Tensor logits, at::Tensor target, at::Tensor lse,
                  at::Tensor gl);
std::vector<at::Tensor> ce_soft_fwd(at::Tensor logits, at::Tensor target,
                                    c10::optional<at::Tensor> lam,
                                    double eps);
at::Tensor ce_soft_bwd(at::Tensor logits, at::Tensor target, at::Tensor lse,
                       at::Tensor gl, c10::optional<at::Tensor> lam,
                       double eps);
std::vector<at::Tensor> topk_acc(at::Tensor logits, at::Tensor target,
                                 int64_t topk);
// mix.hip
at::Tensor batch_mix(at::Tensor x, int64_t mode, double lam, int64_t y0,
                     int64_t y1, int64_t x0, int64_t x1);
// conv.hip
at::Tensor conv2d_fwd_v1(at::Tensor x, at::Tensor w, at::Tensor y,
                         int64_t Ho, int64_t Wo, int64_t sh, int64_t sw,
                         int64_t ph, int64_t pw, int64_t dh, int64_t dw,
                         int64_t groups);
at::Tensor conv2d_fwd(at::Tensor x, at::Tensor w, int64_t sh, int64_t sw,
                      int64_t ph, int64_t pw, int64_t dh, int64_t dw,
                      int64_t groups);
std::vector<at::Tensor> conv2d_fwd_bn(at::Tensor x, at::Tensor w, int64_t sh,
                                      int64_t sw, int64_t ph, int64_t pw,
                                      int64_t dh, int64_t dw, int64_t groups);
std::vector<at::Tensor> conv2d_fwd_halo_dbg(at::Tensor x, at::Tensor w,
                                            bool emit, bool halo);
bool conv3x3_halo_admits(int64_t N, int64_t H, int64_t W);
at::Tensor conv2d_dgrad(at::Tensor gy, at::Tensor w, int64_t H, int64_t W,
                        int64_t sh, int64_t sw, int64_t ph, int64_t pw,
                        int64_t dh, int64_t dw, int64_t groups,
                        c10::optional<at::Tensor> pre, int64_t pre_kind);
std::tuple<std::string, int64_t, bool> conv2d_dgrad_route(
    at::Tensor gy, at::Tensor w, int64_t H, int64_t W, int64_t sh, int64_t sw,
    int64_t ph, int64_t pw, int64_t dh, int64_t dw, int64_t groups,
    c10::optional<at::Tensor> into);

std::tuple<at::Tensor, int64_t> conv2d_dgrad_acc(
    at::Tensor gy, at::Tensor w, int64_t H, int64_t W, int64_t sh, int64_t sw,
    int64_t ph, int64_t pw, int64_t dh, int64_t dw, int64_t groups,
    at::Tensor into, c10::optional<at::Tensor> pre, int64_t pre_kind);

std::tuple<at::Tensor, int64_t> conv2d_dgrad_prep(
    at::Tensor w, int64_t Kt0, int64_t sh, int64_t sw, int64_t ph,
    int64_t pw, int64_t dh, int64_t dw, int64_t groups);
at::Tensor gemm_nt(at::Tensor a, at::Tensor b);
at::Tensor conv2d_fwd_v2(at::Tensor x, at::Tensor w, int64_t sh, int64_t sw,
                         int64_t ph, int64_t pw, int64_t dh, int64_t dw);
at::Tensor weight_flip_t(at::Tensor w, int64_t groups);
at::Tensor dilate_nhwc(at::Tensor x, int64_t sh, int64_t sw);
at::Tensor pad_channels(at::Tensor x, int64_t Cn);
at::Tensor conv2d_wgrad(at::Tensor gy, at::Tensor x, int64_t R, int64_t S,
                        int64_t sh, int64_t sw, int64_t ph, int64_t pw,
                        int64_t dh, int64_t dw, int64_t groups);
std::tuple<std::string, int64_t, int64_t, std::string> conv2d_wgrad_route(
    at::Tensor gy, at::Tensor x, int64_t R, int64_t S, int64_t sh, int64_t sw,
    int64_t ph, int64_t pw, int64_t dh, int64_t dw, int64_t groups);
// depthwise.hip
at::Tensor dwconv_fwd(at::Tensor x, at::Tensor w, int64_t sh, int64_t sw,
                      int64_t ph, int64_t pw);
at::Tensor dwconv_dgrad(at::Tensor gy, at::Tensor w, int64_t H, int64_t W,
                        int64_t sh, int64_t sw, int64_t ph, int64_t pw);
at::Tensor dwconv_wgrad(at::Tensor gy, at::Tensor x, int64_t R, int64_t S,
                        int64_t sh, int64_t sw, int64_t ph, int64_t pw);
// attention.hip
at::Tensor mhsa_fwd(at::Tensor q, at::Tensor k, at::Tensor vt, at::Tensor rw,
                    at::Tensor rh, int64_t H, int64_t W,
                    c10::optional<at::Tensor> pout, int64_t heads,
                    int64_t qpix, int64_t kpix, double scale);
std::vector<at::Tensor> mhsa_bwd(at::Tensor dO, at::Tensor P, at::Tensor q,
                                 at::Tensor kt, at::Tensor v,
                                 at::Tensor rel_w, at::Tensor rel_h,
                                 int64_t H, int64_t W, int64_t heads,
                                 int64_t qpix, int64_t kqoff, int64_t vpix,
                                 int64_t opix, double scale,
                                 at::Tensor dqk_out, at::Tensor dv_out);
at::Tensor mhsa_rel_tables(at::Tensor q, at::Tensor rel, int64_t rows,
                           int64_t heads, int64_t L, int64_t qpix,
                           double scale);
// augment.hip
at::Tensor aug_crop_flip_norm(at::Tensor raw, at::Tensor meta, int64_t S,
                              std::vector<double> mean,
                              std::vector<double> std, at::ScalarType dtype);
// det_reduce.hip
void set_deterministic(bool on);
bool is_deterministic();
// sgd.hip
void sgd_step(at::Tensor table, double lr, double momentum,
              double dampening, double weight_decay, bool nesterov);
void sgd_step_dev(at::Tensor table, at::Tensor lr_dev, double momentum,
                  double dampening, double weight_decay, bool nesterov);
// lars.hip
void lars_step(at::Tensor table, int64_t nchunks, at::Tensor part,
               at::Tensor sqnorm, at::Tensor q, double lr, double momentum,
               double dampening, double weight_decay, bool nesterov,
               double trust_coef, double eps);
void lars_step_dev(at::Tensor table, int64_t nchunks, at::Tensor part,
                   at::Tensor sqnorm, at::Tensor q, at::Tensor lr_dev,
                   double momentum, double dampening, double weight_decay,
                   bool nesterov, double trust_coef, double eps);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("relu_fwd", &relu_fwd);
  m.def("relu_bwd", &relu_bwd);
  m.def("add_relu_fwd", &add_relu_fwd);
  m.def("se_scale_fwd", &se_scale_fwd);
  m.def("dropout_fwd", &dropout_fwd);
  m.def("dropout_fwd_dev", &dropout_fwd_dev);
  m.def("se_scale_bwd", &se_scale_bwd);
  m.def("bn_sums", &bn_sums);
  m.def("bn_reduce_partials", &bn_reduce_partials);
  m.def("bn_stats", &bn_stats, py::arg("x"), py::arg("gamma"), py::arg("beta"),
        py::arg("rm") = py::none(), py::arg("rv") = py::none(),
        py::arg("momentum") = 0.1, py::arg("eps") = 1e-5,
        py::arg("training") = true, py::arg("part") = py::none());
  m.def("bn_apply_act", &bn_apply_act, py::arg("x"), py::arg("scale"),
        py::arg("shift"), py::arg("act"), py::arg("res") = py::none());
  m.def("bn_apply_act_mask", &bn_apply_act_mask, py::arg("x"),
        py::arg("scale"), py::arg("shift"), py::arg("act"), py::arg("res"),
        py::arg("res_scale") = py::none(), py::arg("res_shift") = py::none());
  m.def("bn_act_maxpool_fwd", &bn_act_maxpool_fwd);
  m.def("bn_pool_bwd_stats", &bn_pool_bwd_stats);
  m.def("bn_pool_bwd_apply", &bn_pool_bwd_apply);
  m.def("bn_pool_bwd", &bn_pool_bwd);
  m.def("bn_bwd_stats", &bn_bwd_stats, py::arg("gy"), py::arg("x"),
        py::arg("res"), py::arg("scale"), py::arg("shift"),
        py::arg("act"));
  m.def("bn_bwd_apply", &bn_bwd_apply, py::arg("gy"), py::arg("x"),
        py::arg("res"), py::arg("mean"), py::arg("rstd"),
        py::arg("gamma"), py::arg("scale"), py::arg("shift"), py::arg("sums"),
        py::arg("total_count"), py::arg("act"), py::arg("training"),
        py::arg("need_gres"));
  m.def("bn_bwd", &bn_bwd, py::arg("gy"), py::arg("x"),
        py::arg("res"), py::arg("mean"), py::arg("rstd"), py::arg("gamma"),
        py::arg("scale"), py::arg("shift"), py::arg("act"),
        py::arg("training"), py::arg("need_gres"),
        py::arg("mask") = py::none());
  m.def("maxpool_fwd", &maxpool_fwd);
  m.def("maxpool_bwd", &maxpool_bwd);
  m.def("gap_fwd", &gap_fwd);
  m.def("gap_bwd", &gap_bwd);
  m.def("avgpool_fwd", &avgpool_fwd);
  m.def("avgpool_bwd", &avgpool_bwd);
  m.def("ce_fwd", &ce_fwd);
  m.def("ce_bwd", &ce_bwd);
  m.def("ce_soft_fwd", &ce_soft_fwd, py::arg("logits"), py::arg("target"),
        py::arg("lam") = py::none(), py::arg("eps") = 0.0);
  m.def("ce_soft_bwd", &ce_soft_bwd, py::arg("logits"), py::arg("target"),
        py::arg("lse"), py::arg("gl"), py::arg("lam") = py::none(),
        py::arg("eps") = 0.0);
  m.def("batch_mix", &batch_mix, py::arg("x"), py::arg("mode"),
        py::arg("lam"), py::arg("y0"), py::arg("y1"), py::arg("x0"),
        py::arg("x1"));
  m.def("topk_acc", &topk_acc);
  m.def("sgd_step", &sgd_step);
  m.def("sgd_step_dev", &sgd_step_dev);
  m.def("lars_step", &lars_step);
  m.def("lars_step_dev", &lars_step_dev);
  m.def("conv2d_fwd", &conv2d_fwd);
  m.def("conv2d_fwd_v1", &conv2d_fwd_v1);
  m.def("conv2d_fwd_bn", &conv2d_fwd_bn);
  m.def("conv2d_fwd_halo_dbg", &conv2d_fwd_halo_dbg, py::arg("x"),
        py::arg("w"), py::arg("emit"), py::arg("halo"));
  m.def("conv3x3_halo_admits", &conv3x3_halo_admits);
  m.def("conv2d_dgrad", &conv2d_dgrad, py::arg("gy"), py::arg("w"),
        py::arg("H"), py::arg("W"), py::arg("sh"), py::arg("sw"),
        py::arg("ph"), py::arg("pw"), py::arg("dh"), py::arg("dw"),
        py::arg("groups"), py::arg("pre") = py::none(),
        py::arg("pre_kind") = -1);
  m.def("conv2d_dgrad_route", &conv2d_dgrad_route, py::arg("gy"),
        py::arg("w"), py::arg("H"), py::arg("W"), py::arg("sh"),
        py::arg("sw"), py::arg("ph"), py::arg("pw"), py::arg("dh"),
        py::arg("dw"), py::arg("groups"), py::arg("into") = py::none());
  m.def("conv2d_dgrad_acc", &conv2d_dgrad_acc);
  m.def("conv2d_dgrad_prep", &conv2d_dgrad_prep);
  m.def("conv2d_wgrad", &conv2d_wgrad);
  m.def("conv2d_wgrad_route", &conv2d_wgrad_route);
  m.def("gemm_nt", &gemm_nt);
  m.def("conv2d_fwd_v2", &conv2d_fwd_v2);
  m.def("weight_flip_t", &weight_flip_t);
  m.def("dilate_nhwc", &dilate_nhwc);
  m.def("pad_channels", &pad_channels);
  m.def("dwconv_fwd", &dwconv_fwd);
  m.def("dwconv_dgrad", &dwconv_dgrad);
  m.def("dwconv_wgrad", &dwconv_wgrad);
  m.def("mhsa_fwd", &mhsa_fwd);
  m.def("mhsa_bwd", &mhsa_bwd);
  m.def("mhsa_rel_tables", &mhsa_rel_tables);
  m.def("aug_crop_flip_norm", &aug_crop_flip_norm);
  m.def("set_deterministic", &set_deterministic);
  m.def("is_deterministic", &is_deterministic);
}
