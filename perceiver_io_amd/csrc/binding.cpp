// PyTorch bindings for the Perceiver IO CDNA4 kernels.  Host-only translation unit
// (g++): validates shapes/dtypes, allocates outputs, and launches on the current HIP
// stream so every call is capturable in a hipGraph.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include "host_api.h"

#include <tuple>
#include <unordered_map>
#include <vector>

using torch::Tensor;
using OptT = c10::optional<Tensor>;

namespace {
hipStream_t stream() { return at::hip::getCurrentHIPStream(); }

#ifndef PIO_CHECKS
#define PIO_CHECKS 0
#endif
// checked builds: the device error words of every checked translation unit (bit 1: a token id
// outside the embedding table, 2: a gather row outside its destination, 4: a class label
// outside [0, V) ∪ {-100}, 8: a PE row index outside its table, 16: a batch_augment crop box that had to be
// clamped into its source image, 32: a rand_augment op word outside its table, 128: an event_compact
// dihedral code outside 0-7); reset clears them
int64_t check_errors(bool reset) {
  return (int64_t)(pio::check_errors_elementwise(reset) | pio::check_errors_optim(reset) |
                   pio::check_errors_mlm_head(reset) | pio::check_errors_mlm_select(reset) |
                   pio::check_errors_ce_head(reset) | pio::check_errors_topk_head(reset) |
                   pio::check_errors_rowgemm(reset) | pio::check_errors_pixel_head(reset) |
                   pio::check_errors_soft_ce_head(reset) | pio::check_errors_augment(reset) |
                   pio::check_errors_randaugment(reset) | pio::check_errors_health(reset) |
                   pio::check_errors_lartpc_prep(reset));
}
bool checked_build() { return PIO_CHECKS != 0; }
// checked builds, outside graph capture: wait for the kernel just launched and raise on any
// device-side index violation (the kernel itself clamped / skipped the access)
void checked_sync(const char* what) {
  if (!PIO_CHECKS) return;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(stream(), &cs);
  if (cs != hipStreamCaptureStatusNone) return;
  (void)hipStreamSynchronize(stream());
  const int64_t e = check_errors(true);
  TORCH_CHECK(e == 0, "checked build: ", what, " saw out-of-range indices (error bits ", e,
              ": 1 token id >= vocab, 2 gather row out of range, 4 label outside [0, V) and != -100, 8 PE row index outside "
              "the position-encoding table, 16 batch_augment crop box outside its source image, 32 rand_augment op word "
              "outside its table)");
}

// deterministic mode (trainer flag ``deterministic``): every reduction that would
// use fp32 atomics with several writers per address runs as a fixed-order split reduction
bool g_det = false;

#define CHECK_CUDA(t) TORCH_CHECK((t).is_cuda(), #t " must be a GPU tensor")
#define CHECK_DT(t, dt) TORCH_CHECK((t).scalar_type() == (dt), #t " has wrong dtype ", (t).scalar_type())

const uint16_t* bfp(const Tensor& t) { CHECK_DT(t, torch::kBFloat16); return reinterpret_cast<const uint16_t*>(t.data_ptr()); }
uint16_t* bfp_mut(Tensor& t) { CHECK_DT(t, torch::kBFloat16); return reinterpret_cast<uint16_t*>(t.data_ptr()); }
const float* f32p(const Tensor& t) { CHECK_DT(t, torch::kFloat32); return t.data_ptr<float>(); }
const float* f32o(const OptT& t) { return t.has_value() ? f32p(*t) : nullptr; }
bool is_bf16(const Tensor& t) {
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16 || t.scalar_type() == torch::kFloat32, "expected bf16/fp32");
  return t.scalar_type() == torch::kBFloat16;
}
float* f32p_mut(Tensor& t) { CHECK_DT(t, torch::kFloat32); return t.data_ptr<float>(); }
// the rows of a 2-D fp32 / bf16 tensor with unit inner stride
pio::RowsIn rows_in(const Tensor& t) { return pio::RowsIn{t.data_ptr(), is_bf16(t), (int)t.stride(0)}; }

// 3-D (B|1, N, >=HD) view with unit inner stride → (batch stride, row stride)
void strides3(const Tensor& t, int B, long long& bs, int& rs) {
  TORCH_CHECK(t.dim() == 3 && t.stride(2) == 1, "attention operand must be 3-D with unit inner stride");
  TORCH_CHECK(t.size(0) == B || t.size(0) == 1, "batch mismatch");
  bs = t.size(0) == 1 ? 0 : t.stride(0);
  rs = (int)t.stride(1);
  TORCH_CHECK(rs % 8 == 0 && (bs % 8 == 0) && (reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0),
              "attention operands need 16-byte aligned rows");
}

// device dropout seed: a 1-element int64 GPU tensor (drawn per forward call, see host_api.h DropCfg)
const int64_t* seed_ptr(const OptT& seed, double p) {
  if (!(p > 0)) return nullptr;
  TORCH_CHECK(seed.has_value(), "dropout > 0 needs a device seed tensor");
  TORCH_CHECK(seed->is_cuda() && seed->scalar_type() == torch::kInt64 && seed->numel() >= 1,
              "dropout seed must be an int64 GPU tensor");
  return seed->data_ptr<int64_t>();
}

pio::DropCfg make_drop(const OptT& seed, int64_t site, double p) {
  TORCH_CHECK(p >= 0 && p < 1, "dropout probability must be in [0, 1)");
  pio::DropCfg d{};
  d.seed = seed_ptr(seed, p);
  d.site = (uint32_t)site;
  d.thresh = p > 0 ? (uint32_t)std::min(4294967295.0, p * 4294967296.0) : 0u;
  d.scale = p > 0 ? (float)(1.0 / (1.0 - p)) : 1.f;
  return d;
}

pio::AttnArgs make_args(const Tensor& q, const Tensor& k, const Tensor& v, const OptT& kmask, int H, int D,
                        double scale, double dropout_p, const OptT& seed, int64_t site) {
  CHECK_CUDA(q); CHECK_CUDA(k); CHECK_CUDA(v);
  pio::AttnArgs a{};
  a.B = (int)std::max(q.size(0), k.size(0));
  a.H = H;
  a.Nq = (int)q.size(1);
  a.Nk = (int)k.size(1);
  TORCH_CHECK(v.size(1) == a.Nk, "K/V length mismatch");
  TORCH_CHECK(D == 16 || D == 32 || D == 64 || D == 128, "head dim must be 16/32/64/128, got ", D);
  TORCH_CHECK(q.size(2) >= H * D && k.size(2) >= H * D && v.size(2) >= H * D, "head columns out of range");
  TORCH_CHECK(k.size(0) == a.B && v.size(0) == a.B, "K/V must carry the full batch");
  a.q = bfp(q); a.k = bfp(k); a.v = bfp(v);
  strides3(q, a.B, a.q_bs, a.q_rs);
  strides3(k, a.B, a.k_bs, a.k_rs);
  strides3(v, a.B, a.v_bs, a.v_rs);
  a.kmask = nullptr;
  if (kmask.has_value()) {
    const Tensor& m = *kmask;
    CHECK_CUDA(m);
    TORCH_CHECK(m.scalar_type() == torch::kBool || m.scalar_type() == torch::kUInt8, "key mask must be bool/uint8");
    TORCH_CHECK(m.is_contiguous() && m.size(0) == a.B && m.size(1) == a.Nk, "key mask must be (B, Nk) contiguous");
    a.kmask = reinterpret_cast<const uint8_t*>(m.data_ptr());
  }
  a.scale = (float)scale;
  a.scale_log2 = (float)(scale * 1.4426950408889634);
  const pio::DropCfg d = make_drop(seed, site, dropout_p);
  a.drop_thresh = d.thresh;
  a.drop_scale = d.scale;
  a.seedp = d.seed;
  a.site = d.site;
  return a;
}
}  // namespace

std::vector<Tensor> attn_fwd(Tensor q, Tensor k, Tensor v, OptT kmask, int64_t H, int64_t D, double scale,
                             double dropout_p, OptT seed, int64_t nsplit, int64_t site) {
  auto a = make_args(q, k, v, kmask, (int)H, (int)D, scale, dropout_p, seed, site);
  auto opts = q.options();
  Tensor O = torch::empty({a.B, a.Nq, H * D}, opts.dtype(torch::kBFloat16));
  Tensor L = torch::empty({a.B, a.Nq, H}, opts.dtype(torch::kFloat32));
  Tensor Op, ML;
  float* opp = nullptr; float* mlp = nullptr;
  if (nsplit > 1) {
    Op = torch::empty({nsplit, a.B, a.Nq, H, D}, opts.dtype(torch::kFloat32));
    ML = torch::empty({nsplit, a.B, a.Nq, H, 2}, opts.dtype(torch::kFloat32));
    opp = Op.data_ptr<float>(); mlp = ML.data_ptr<float>();
  }
  pio::attn_fwd_launch(a, (int)D, bfp_mut(O), L.data_ptr<float>(), opp, mlp, (int)std::max<int64_t>(1, nsplit), stream());
  return {O, L};
}

// head-averaged attention weights of a forward (attn_weights.hip): q (B|1, Nq, >= H·D), k (B, Nk,
// >= H·D) bf16 views as attn_fwd takes them, lse (B, Nq, H) fp32 as attn_fwd returned it →
// (avg (B, Nq, Nk) fp32 | None, mass (B, Nk) fp32 | None).  Inference only.
std::tuple<OptT, OptT> attn_weights(Tensor q, Tensor k, OptT kmask, Tensor lse, int64_t H, int64_t D, double scale,
                                    bool want_avg, bool want_mass) {
  TORCH_CHECK(want_avg || want_mass, "attn_weights: at least one of avg / mass must be requested");
  auto a = make_args(q, k, k, kmask, (int)H, (int)D, scale, 0.0, c10::nullopt, 0);
  CHECK_CUDA(lse);
  TORCH_CHECK(lse.is_contiguous() && lse.dim() == 3 && lse.size(0) == a.B && lse.size(1) == a.Nq && lse.size(2) == H,
              "attn_weights: lse must be (B, Nq, H) contiguous");
  TORCH_CHECK(a.B <= 65535 && a.Nk <= (1 << 26), "attn_weights: at most 65535 samples and 2^26 keys per call");
  // the kernel indexes a sample's LSE rows with 32-bit offsets
  TORCH_CHECK((int64_t)a.Nq * H < (int64_t(1) << 31), "attn_weights: Nq * H must be below 2^31");
  auto opts = q.options().dtype(torch::kFloat32);
  const int nchunks = pio::attn_weights_chunks(a.B, a.Nq, a.Nk);
  OptT avg, mass;
  Tensor part;
  if (want_avg) avg = torch::empty({a.B, a.Nq, a.Nk}, opts);
  if (want_mass) {
    mass = torch::empty({a.B, a.Nk}, opts);
    if (nchunks > 1) part = torch::empty({a.B, nchunks, a.Nk}, opts);
  }
  pio::attn_weights_launch(a, (int)D, f32p(lse), want_avg ? avg->data_ptr<float>() : nullptr,
                           want_mass ? mass->data_ptr<float>() : nullptr,
                           part.defined() ? part.data_ptr<float>() : nullptr, nchunks, stream());
  return {avg, mass};
}

// returns (dq, dk, dv) fp32; dq is per batch even when q is batch-broadcast.  Optional
namespace {
pio::SlabJob make_job(const OptT& slab, std::vector<Tensor>& dsts, const std::vector<int64_t>& offs);
}  // namespace

// *_out tensors (B, N, >=HD views, unit inner stride) let the results land in packed buffers;
// a dq_out view must be batch-dense (batch stride == Nq * row stride); it needs no zero fill
// (the launcher clears it itself when several key blocks accumulate into it).  delta_in ((B, Nq, H) fp32 rowsum(dO∘O), e.g. from post_attn_bwd)
// skips the delta pass.
std::vector<Tensor> attn_bwd(Tensor q, Tensor k, Tensor v, OptT kmask, Tensor o, Tensor dO, Tensor lse, OptT delta_in,
                             int64_t H, int64_t D, double scale, double dropout_p, OptT seed, OptT dq_out,
                             OptT dk_out, OptT dv_out, bool kv_accumulate, int64_t site, bool dq_zeroed,
                             bool kv_zeroed, OptT job_slab, std::vector<Tensor> job_dsts, std::vector<int64_t> job_offs) {
  auto a = make_args(q, k, v, kmask, (int)H, (int)D, scale, dropout_p, seed, site);
  // job (optional): the previous kernel's slab reduction, carried by the bf16 variant (else a
  // standalone launch first)
  const pio::SlabJob job = make_job(job_slab, job_dsts, job_offs);
  TORCH_CHECK(dO.is_contiguous() && o.is_contiguous(), "O / dO must be contiguous (B, Nq, H*D)");
  auto f32 = q.options().dtype(torch::kFloat32);
  if (dq_out.has_value() && dq_out->scalar_type() == torch::kBFloat16) {
    // bf16 outputs (all three, stored once each): the self-attention backward feeding the
    // chain-layout layer-boundary kernel, which reads them as bf16 operands
    TORCH_CHECK(dk_out.has_value() && dv_out.has_value() && dk_out->scalar_type() == torch::kBFloat16 &&
                    dv_out->scalar_type() == torch::kBFloat16 && delta_in.has_value() && !kv_accumulate,
                "bf16 attn_bwd outputs: dq/dk/dv all bf16, delta given, no accumulation");
    Tensor dq = *dq_out, dk = *dk_out, dv = *dv_out;
    TORCH_CHECK(dq.stride(2) == 1 && dk.stride(2) == 1 && dv.stride(2) == 1, "dq/dk/dv need unit inner stride");
    Tensor delta = *delta_in;
    TORCH_CHECK(delta.is_contiguous() && delta.numel() == (int64_t)a.B * a.Nq * H, "delta must be (B, Nq, H)");
    CHECK_DT(delta, torch::kFloat32);
    if (pio::attn_bwd_bf16_ok(a, (int)D)) {
      pio::attn_bwd_bf16_launch(a, (int)D, bfp(dO), f32p(lse), delta.data_ptr<float>(), bfp_mut(dq), dq.stride(0),
                                (int)dq.stride(1), bfp_mut(dk), dk.stride(0), (int)dk.stride(1), bfp_mut(dv),
                                dv.stride(0), (int)dv.stride(1), job, stream());
    } else {  // shape not covered by the bf16 variant: fp32, then narrowed
      if (job.slab) pio::slab_reduce_launch(job, stream());
      std::vector<Tensor> nd;
      auto r = attn_bwd(q, k, v, kmask, o, dO, lse, delta_in, H, D, scale, dropout_p, seed, c10::nullopt, c10::nullopt,
                        c10::nullopt, false, site, false, false, c10::nullopt, nd, {});
      dq.copy_(r[0]); dk.copy_(r[1]); dv.copy_(r[2]);
    }
    return {dq, dk, dv};
  }
  if (job.slab) pio::slab_reduce_launch(job, stream());
  Tensor dq = dq_out.has_value() ? *dq_out : torch::empty({a.B, a.Nq, H * D}, f32);
  Tensor dk = dk_out.has_value() ? *dk_out : torch::empty({a.B, a.Nk, H * D}, f32);
  Tensor dv = dv_out.has_value() ? *dv_out : torch::empty({a.B, a.Nk, H * D}, f32);
  TORCH_CHECK(dq.stride(2) == 1 && dk.stride(2) == 1 && dv.stride(2) == 1, "dq/dk/dv need unit inner stride");
  TORCH_CHECK(dq.size(0) == a.B && dq.stride(0) == a.Nq * dq.stride(1), "dq must be batch-dense");
  CHECK_DT(dq, torch::kFloat32); CHECK_DT(dk, torch::kFloat32); CHECK_DT(dv, torch::kFloat32);
  Tensor delta;
  if (delta_in.has_value()) {
    delta = *delta_in;
    TORCH_CHECK(delta.is_contiguous() && delta.numel() == (int64_t)a.B * a.Nq * H, "delta must be (B, Nq, H)");
    CHECK_DT(delta, torch::kFloat32);
  } else {
    delta = torch::empty({a.B, a.Nq, H}, f32);
  }
  auto rows3 = [](Tensor& t) { return pio::Rows3{t.data_ptr<float>(), t.stride(0), (int)t.stride(1)}; };
  pio::AttnBwdArgs b{};
  b.a = a;
  b.O = bfp(o);
  b.dO = bfp(dO);
  b.LSE = f32p(lse);
  b.delta = delta.data_ptr<float>();
  b.dk = rows3(dk);
  b.dv = rows3(dv);
  b.compute_delta = !delta_in.has_value();
  b.kv_acc = kv_accumulate;
  const int nkb = pio::attn_bwd_key_blocks(a.Nk, (int)D);
  if (g_det && nkb > 1) {  // one dQ partial slice per key block, summed in a fixed order
    Tensor part = torch::empty({nkb, a.B, a.Nq, H * D}, f32);
    b.dq = pio::Rows3{part.data_ptr<float>(), (long long)a.Nq * H * D, (int)(H * D)};
    b.dq_kbs = (long long)a.B * a.Nq * H * D;
    b.qsplit_ok = 0;
    b.dq_zeroed = 0;
    pio::attn_bwd_launch(b, (int)D, stream());
    dq.narrow(2, 0, H * D).copy_(part.sum(0));
    return {dq, dk, dv};
  }
  b.dq = rows3(dq);
  b.dq_kbs = 0;
  b.qsplit_ok = g_det ? 0 : 1;
  b.dq_zeroed = (dq_zeroed ? 1 : 0) | (kv_zeroed ? 2 : 0);
  pio::attn_bwd_launch(b, (int)D, stream());
  return {dq, dk, dv};
}

// pe (optional, SURVEY K-03): x holds only the npix pixel channels of each row and row r's
// input is pe[r mod rows(pe)] — or pe[pe_index[r]] when the (R,) int64 pe_index is given (sparse
// images) — with the pixels added into its npix leading (zero) columns; pe is (M, pe_rs) fp32
// contiguous with pe_rs a multiple of 8, ≥ Kin = w.size(1)
namespace {
pio::PeSplit pe_split(const OptT& pe, const Tensor& x, int R, int Kin, const OptT& pe_index) {
  pio::PeSplit ps{};
  ps.M = 1;
  TORCH_CHECK(!pe_index.has_value() || pe.has_value(), "pe_index needs a pe table");
  if (!pe.has_value()) return ps;
  CHECK_DT(*pe, torch::kFloat32);
  TORCH_CHECK(pe->dim() == 2 && pe->is_contiguous() && pe->size(1) % 8 == 0 && pe->size(1) >= Kin,
              "pe must be (M, pe_rs) contiguous fp32, pe_rs a multiple of 8 and >= Kin");
  if (pe_index.has_value()) {
    CHECK_DT(*pe_index, torch::kInt64);
    TORCH_CHECK(pe_index->is_contiguous() && pe_index->numel() == R, "pe_index must be R contiguous int64 rows");
    ps.idx = reinterpret_cast<const long long*>(pe_index->data_ptr<int64_t>());
  } else {
    TORCH_CHECK(R % pe->size(0) == 0, "rows must be a multiple of the PE rows");
  }
  TORCH_CHECK(reinterpret_cast<uintptr_t>(pe->data_ptr()) % 16 == 0, "pe must be 16-byte aligned");
  ps.pe = pe->data_ptr<float>();
  ps.pe_rs = (int)pe->size(1);
  ps.M = (int)pe->size(0);
  ps.npix = (int)x.size(1);
  TORCH_CHECK(ps.npix <= Kin, "more pixel channels than inputs");
  return ps;
}
}  // namespace

// kin (optional): the logical input width when w's rows are zero padded past it (w (N, ≥ kin))
std::vector<Tensor> ln_linear_fwd(Tensor x, OptT lnw, OptT lnb, double eps, Tensor w, OptT bias, int64_t act, OptT res,
                                  bool out_bf16, bool save_stats, OptT pe, int64_t kin, OptT pe_index) {
  CHECK_CUDA(x); CHECK_CUDA(w);
  TORCH_CHECK(x.dim() == 2 && x.stride(1) == 1, "x must be 2-D rows");
  const int R = (int)x.size(0), N = (int)w.size(0);
  const int Kin = kin >= 0 ? (int)kin : (int)w.size(1);
  TORCH_CHECK(w.dim() == 2 && w.is_contiguous() && w.size(1) >= Kin, "w must be (N, >= Kin) contiguous");
  TORCH_CHECK(pe.has_value() || x.size(1) == Kin, "x must be (R, Kin)");
  TORCH_CHECK(Kin <= 256, "Kin > 256 unsupported");
  pio::LnLinearFwdArgs a{};
  a.ps = pe_split(pe, x, R, Kin, pe_index);
  auto opts = x.options();
  Tensor y = torch::empty({R, N}, opts.dtype(out_bf16 ? torch::kBFloat16 : torch::kFloat32));
  Tensor mean, rstd;
  if (save_stats && lnw.has_value()) {
    mean = torch::empty({R}, opts.dtype(torch::kFloat32));
    rstd = torch::empty({R}, opts.dtype(torch::kFloat32));
    a.mean = mean.data_ptr<float>();
    a.rstd = rstd.data_ptr<float>();
  }
  if (res.has_value()) { a.res = f32p(*res); a.res_rs = (int)res->stride(0); TORCH_CHECK(res->stride(1) == 1); }
  a.X = rows_in(x);
  a.R = R;
  a.Kin = Kin;
  a.lnw = f32o(lnw);
  a.lnb = f32o(lnb);
  a.eps = (float)eps;
  a.W = bfp(w);
  a.w_rs = (int)w.size(1);
  a.bias = f32o(bias);
  a.N = N;
  a.act = (int)act;
  a.Y = pio::RowsOut{y.data_ptr(), out_bf16, N};
  pio::ln_linear_fwd_launch(a, stream());
  if (a.ps.idx) checked_sync("ln_linear_fwd (pe_index)");
  std::vector<Tensor> out{y};
  if (a.mean) { out.push_back(mean); out.push_back(rstd); }
  return out;
}

std::vector<Tensor> post_attn_fwd(Tensor o, Tensor x, Tensor wo, Tensor bo, Tensor g2, Tensor be2, double eps,
                                  Tensor w1, Tensor b1, Tensor w2, Tensor b2, OptT seed, int64_t site, double p) {
  TORCH_CHECK(o.is_contiguous() && x.is_contiguous(), "o/x must be contiguous (R, C)");
  const int R = (int)o.size(0), C = (int)o.size(1), Rx = (int)x.size(0);
  TORCH_CHECK(x.size(1) == C && Rx > 0 && R % Rx == 0, "x must be (R / k, C): row r adds x[r % rows(x)]");
  TORCH_CHECK(C == 32 || C == 64 || C == 128, "post_attn supports C in {32, 64, 128}");
  auto f32 = x.options().dtype(torch::kFloat32);
  Tensor z = torch::empty({R, C}, f32), y = torch::empty({R, C}, f32);
  Tensor m = torch::empty({R}, f32), r = torch::empty({R}, f32);
  Tensor u = torch::empty({R, C}, x.options().dtype(torch::kBFloat16));
  pio::PostAttnFwdArgs a{};
  a.O = bfp(o);
  a.X = f32p(x);
  a.p.Wo = bfp(wo);
  a.p.bo = f32p(bo);
  a.p.g2 = f32p(g2);
  a.p.be2 = f32p(be2);
  a.p.eps = (float)eps;
  a.p.W1 = bfp(w1);
  a.p.b1 = f32p(b1);
  a.p.W2 = bfp(w2);
  a.p.b2 = f32p(b2);
  a.Z = z.data_ptr<float>();
  a.s.Ysave = y.data_ptr<float>();
  a.s.mean2 = m.data_ptr<float>();
  a.s.rstd2 = r.data_ptr<float>();
  a.s.Usave = bfp_mut(u);
  a.R = R;
  a.Rx = Rx;
  a.dr = make_drop(seed, site, p);
  pio::post_attn_fwd_launch(a, C, stream());
  return {z, y, m, r, u};
}

// self-attention layer boundary l → l+1: post-attention block of layer l, then LN1 + packed QKV
// projection of layer l+1 from the same tile.  Returns (z, y, mean2, rstd2, u, qkv, mean1, rstd1).
std::vector<Tensor> post_attn_ln_linear_fwd(Tensor o, Tensor x, Tensor wo, Tensor bo, Tensor g2, Tensor be2, double eps,
                                            Tensor w1, Tensor b1, Tensor w2, Tensor b2, Tensor lnw, Tensor lnb,
                                            Tensor wq, Tensor bq, OptT seed, int64_t site, double p) {
  TORCH_CHECK(o.is_contiguous() && x.is_contiguous(), "o/x must be contiguous (R, C)");
  const int R = (int)o.size(0), C = (int)o.size(1);
  const int Rx = (int)x.size(0);
  TORCH_CHECK(x.size(1) == C && Rx > 0 && R % Rx == 0, "x must be (R / k, C): row r adds x[r % rows(x)]");
  TORCH_CHECK(C == 32 || C == 64 || C == 128, "post_attn supports C in {32, 64, 128}");
  TORCH_CHECK(wq.is_contiguous() && wq.size(0) == 3 * C && wq.size(1) == C && bq.numel() == 3 * C,
              "wq must be the packed (3C, C) in-projection");
  TORCH_CHECK(lnw.numel() == C && lnb.numel() == C, "LN1 affine must have C entries");
  auto f32 = x.options().dtype(torch::kFloat32);
  auto b16 = x.options().dtype(torch::kBFloat16);
  Tensor z = torch::empty({R, C}, f32), y = torch::empty({R, C}, f32);
  Tensor m = torch::empty({R}, f32), r = torch::empty({R}, f32), u = torch::empty({R, C}, b16);
  Tensor qkv = torch::empty({R, 3 * C}, b16), m1 = torch::empty({R}, f32), r1 = torch::empty({R}, f32);
  pio::PostAttnFwdArgs a{};
  a.O = bfp(o);
  a.X = f32p(x);
  a.p.Wo = bfp(wo);
  a.p.bo = f32p(bo);
  a.p.g2 = f32p(g2);
  a.p.be2 = f32p(be2);
  a.p.eps = (float)eps;
  a.p.W1 = bfp(w1);
  a.p.b1 = f32p(b1);
  a.p.W2 = bfp(w2);
  a.p.b2 = f32p(b2);
  a.Z = z.data_ptr<float>();
  a.s.Ysave = y.data_ptr<float>();
  a.s.mean2 = m.data_ptr<float>();
  a.s.rstd2 = r.data_ptr<float>();
  a.s.Usave = bfp_mut(u);
  a.R = R;
  a.Rx = Rx;
  a.next.lnw = f32p(lnw);
  a.next.lnb = f32p(lnb);
  a.next.Wq = bfp(wq);
  a.next.bq = f32p(bq);
  a.next.QKVn = bfp_mut(qkv);
  a.next.mean1 = m1.data_ptr<float>();
  a.next.rstd1 = r1.data_ptr<float>();
  a.next.nq = 3 * C;
  a.dr = make_drop(seed, site, p);
  pio::post_attn_ln_linear_fwd_launch(a, C, stream());
  return {z, y, m, r, u, qkv, m1, r1};
}

// fused latent self-attention layer forward (C = 64, H = 4, N ≤ 512 (> 256: 16-byte aligned
// operands, the chain kernel), N % 64 == 0, no attention
// dropout; residual dropout allowed): qkv (R, 3C) bf16 of this layer, x (R, C) fp32 its input →
// [o, lse, z, y, m2, r2, u] (+ [qkv, mean1, rstd1] of the next layer when lnw/lnb/wq/bq given)
std::vector<Tensor> sa_layer_fwd(Tensor qkv, Tensor x, int64_t N, double scale, Tensor wo, Tensor bo, Tensor g2,
                                 Tensor be2, double eps, Tensor w1, Tensor b1, Tensor w2, Tensor b2, OptT lnw, OptT lnb,
                                 OptT wq, OptT bq, OptT seed, int64_t site, double p) {
  const int C = 64, H = 4;
  TORCH_CHECK(qkv.is_contiguous() && x.is_contiguous(), "qkv/x must be contiguous");
  const int R = (int)x.size(0);
  TORCH_CHECK(x.size(1) == C && qkv.size(0) == R && qkv.size(1) == 3 * C, "sa_layer_fwd: C = 64, qkv (R, 192)");
  TORCH_CHECK(N > 0 && N <= 512 && N % 64 == 0 && R % N == 0, "sa_layer_fwd: N <= 512, N % 64 == 0, R = B·N");
  const bool next = wq.has_value();
  if (next)
    TORCH_CHECK(lnw.has_value() && lnb.has_value() && bq.has_value() && wq->is_contiguous() &&
                    (wq->size(0) == 3 * C || wq->size(0) == 2 * C || wq->size(0) == C) && wq->size(1) == C &&
                    bq->numel() == wq->size(0) &&
                    lnw->numel() == C && lnb->numel() == C,
                "sa_layer_fwd: next LN + projection (packed QKV (3C, C), K/V (2C, C) or a query projection (C, C))");
  const int nq = next ? (int)wq->size(0) : 3 * C;
  auto f32 = x.options().dtype(torch::kFloat32);
  auto b16 = x.options().dtype(torch::kBFloat16);
  Tensor o = torch::empty({R / N, N, C}, b16), lse = torch::empty({R / N, N, H}, f32);
  Tensor z = torch::empty({R, C}, f32), y = torch::empty({R, C}, f32);
  Tensor m = torch::empty({R}, f32), r = torch::empty({R}, f32), u = torch::empty({R, C}, b16);
  Tensor qn, m1, r1;
  if (next) { qn = torch::empty({R, nq}, b16); m1 = torch::empty({R}, f32); r1 = torch::empty({R}, f32); }
  pio::SaLayerFwdArgs a{};
  a.QKV = bfp(qkv);
  a.N = (int)N;
  a.scale_log2 = (float)(scale * 1.4426950408889634);
  a.O = bfp_mut(o);
  a.LSE = lse.data_ptr<float>();
  a.X = f32p(x);
  a.p.Wo = bfp(wo);
  a.p.bo = f32p(bo);
  a.p.g2 = f32p(g2);
  a.p.be2 = f32p(be2);
  a.p.eps = (float)eps;
  a.p.W1 = bfp(w1);
  a.p.b1 = f32p(b1);
  a.p.W2 = bfp(w2);
  a.p.b2 = f32p(b2);
  a.Z = z.data_ptr<float>();
  a.s.Ysave = y.data_ptr<float>();
  a.s.mean2 = m.data_ptr<float>();
  a.s.rstd2 = r.data_ptr<float>();
  a.s.Usave = bfp_mut(u);
  a.R = R;
  if (next) {
    a.next.lnw = f32p(*lnw);
    a.next.lnb = f32p(*lnb);
    a.next.Wq = bfp(*wq);
    a.next.bq = f32p(*bq);
    a.next.QKVn = bfp_mut(qn);
    a.next.mean1 = m1.data_ptr<float>();
    a.next.rstd1 = r1.data_ptr<float>();
  }
  a.next.nq = nq;
  a.dr = make_drop(seed, site, p);
  TORCH_CHECK(pio::sa_layer_fwd_launch(a, stream()), "sa_layer_fwd: every operand must be 16-byte aligned");
  if (next) return {o, lse, z, y, m, r, u, qn, m1, r1};
  return {o, lse, z, y, m, r, u};
}


// sync words of the persistent kernels (csrc/persist.hip): one zero-initialised buffer per
// (device, stream), allocated on the first launch on that stream (never during a stream capture:
// nullptr then, the caller runs the per-layer kernels), reset to zero by the last workgroup of
// every launch — launches on one stream run one after another, so they can share it
unsigned* persist_sync_buffer(const Tensor& like, int words) {
  // grown buffers are kept alive too: a captured graph may still name an older one
  static std::unordered_map<uint64_t, std::vector<Tensor>> bufs;
  hipStream_t st = stream();
  const uint64_t key = reinterpret_cast<uint64_t>(st) ^ ((uint64_t)like.get_device() << 56);
  auto& v = bufs[key];
  if (!v.empty() && v.back().numel() >= words) return reinterpret_cast<unsigned*>(v.back().data_ptr<int>());
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return nullptr;
  // the zero fill runs on the current stream: ordered before every launch that uses the buffer
  v.push_back(torch::zeros({std::max(words, 1 << 14)}, like.options().dtype(torch::kInt32)));
  return reinterpret_cast<unsigned*>(v.back().data_ptr<int>());
}

// persistent self-attention block forward (csrc/persist.hip): every layer of a C = 64, H = 4
// block with N ≤ 256 latents in ONE launch.  Per layer i: wo..b2 (its post-attention block) and,
// for i < L - 1, the next layer's (lnw, lnb, wq, bq); the last layer optionally gets the next
// cross-attention layer's LN + query (64 rows) or K/V (128 rows) projection as an L-th entry.  Returns, per layer, [o, lse, z, y, m2, r2, u] + [qkv_n, mean_n, rstd_n] when that
// layer has a next projection.  Empty list: the operands do not qualify (the caller runs the
// per-layer kernels).
std::vector<Tensor> sa_block_fwd(Tensor qkv0, Tensor x0, int64_t N, double scale, double eps, std::vector<Tensor> wo,
                                 std::vector<Tensor> bo, std::vector<Tensor> g2, std::vector<Tensor> be2,
                                 std::vector<Tensor> w1, std::vector<Tensor> b1, std::vector<Tensor> w2,
                                 std::vector<Tensor> b2, std::vector<Tensor> lnw, std::vector<Tensor> lnb,
                                 std::vector<Tensor> wq, std::vector<Tensor> bq, OptT seed, double p) {
  const int C = 64, H = 4;
  const int L = (int)wo.size();
  TORCH_CHECK(L >= 1 && L <= pio::kPersistMaxLayers, "sa_block_fwd: 1..8 layers");
  TORCH_CHECK(bo.size() == (size_t)L && g2.size() == (size_t)L && be2.size() == (size_t)L && w1.size() == (size_t)L &&
                  b1.size() == (size_t)L && w2.size() == (size_t)L && b2.size() == (size_t)L,
              "sa_block_fwd: one post-attention parameter set per layer");
  const int nn = (int)wq.size();
  TORCH_CHECK((nn == L - 1 || nn == L) && lnw.size() == (size_t)nn && lnb.size() == (size_t)nn && bq.size() == (size_t)nn,
              "sa_block_fwd: L - 1 next projections (+ an optional last query projection)");
  TORCH_CHECK(qkv0.is_contiguous() && x0.is_contiguous(), "sa_block_fwd: contiguous qkv / x");
  const int R = (int)x0.size(0);
  TORCH_CHECK(x0.size(1) == C && qkv0.size(0) == R && qkv0.size(1) == 3 * C, "sa_block_fwd: C = 64, qkv (R, 192)");
  CHECK_DT(x0, torch::kFloat32);
  if (N <= 0 || N > 256 || N % 64 != 0 || R % N != 0 || (long long)R * 3 * C * 2 >= (1LL << 31)) return {};
  auto al = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
  if (!al(qkv0.data_ptr()) || !al(x0.data_ptr())) return {};
  auto f32 = x0.options().dtype(torch::kFloat32);
  auto b16 = x0.options().dtype(torch::kBFloat16);
  const int B = R / (int)N;
  unsigned* sync = persist_sync_buffer(x0, pio::persist_sync_words(B));
  if (sync == nullptr) return {};
  pio::SABlockFwdArgs a{};
  a.QKV0 = bfp(qkv0);
  a.X0 = f32p(x0);
  a.sync = sync;
  a.L = L; a.N = (int)N; a.R = R;
  a.scale_log2 = (float)(scale * 1.4426950408889634);
  a.eps = (float)eps;
  a.dr = make_drop(seed, 0, p);
  std::vector<Tensor> out;
  for (int i = 0; i < L; ++i) {
    pio::SAFwdLayer& y = a.ly[i];
    for (const Tensor* t : {&wo[i], &w1[i], &w2[i]})
      TORCH_CHECK(t->is_contiguous() && t->size(0) == C && t->size(1) == C, "sa_block_fwd: (C, C) weights");
    y.Wo = bfp(wo[i]); y.W1 = bfp(w1[i]); y.W2 = bfp(w2[i]);
    y.bo = f32p(bo[i]); y.g2 = f32p(g2[i]); y.be2 = f32p(be2[i]); y.b1 = f32p(b1[i]); y.b2 = f32p(b2[i]);
    if (!al(y.Wo) || !al(y.W1) || !al(y.W2) || !al(y.g2) || !al(y.be2) || !al(y.bo) || !al(y.b1) || !al(y.b2)) return {};
    Tensor o = torch::empty({B, (int)N, C}, b16), lse = torch::empty({B, (int)N, H}, f32);
    Tensor z = torch::empty({R, C}, f32), yy = torch::empty({R, C}, f32);
    Tensor m = torch::empty({R}, f32), r = torch::empty({R}, f32), u = torch::empty({R, C}, b16);
    y.O = bfp_mut(o); y.LSE = lse.data_ptr<float>(); y.Z = z.data_ptr<float>(); y.Y = yy.data_ptr<float>();
    y.mean2 = m.data_ptr<float>(); y.rstd2 = r.data_ptr<float>(); y.U = bfp_mut(u);
    out.insert(out.end(), {o, lse, z, yy, m, r, u});
    if (i < nn) {
      const int nq = (int)wq[i].size(0);
      TORCH_CHECK(wq[i].is_contiguous() && wq[i].size(1) == C && (nq == 3 * C || (i == L - 1 && (nq == C || nq == 2 * C))) &&
                      bq[i].numel() == nq && lnw[i].numel() == C && lnb[i].numel() == C,
                  "sa_block_fwd: next projection (3C, C) (the last layer's may be a (C, C) query or (2C, C) K/V projection)");
      y.Wq = bfp(wq[i]); y.lnw = f32p(lnw[i]); y.lnb = f32p(lnb[i]); y.bq = f32p(bq[i]); y.nq = nq;
      if (!al(y.Wq) || !al(y.lnw) || !al(y.lnb) || !al(y.bq)) return {};
      Tensor qn = torch::empty({R, nq}, b16), m1 = torch::empty({R}, f32), r1 = torch::empty({R}, f32);
      y.QKVn = bfp_mut(qn); y.mean1n = m1.data_ptr<float>(); y.rstd1n = r1.data_ptr<float>();
      out.insert(out.end(), {qn, m1, r1});
    }
  }
  if (!pio::sa_block_fwd_launch(a, stream())) return {};
  return out;
}

unsigned persist_errors(bool reset) { return pio::persist_errors(reset); }

namespace {
pio::SlabJob make_job(const OptT& slab, std::vector<Tensor>& dsts, const std::vector<int64_t>& offs);
}  // namespace

// ---- per-sample latent-block kernels (csrc/sample_block.hip): C ∈ {64, 128}, H = 4, N = 32 ----
namespace {
constexpr int kSBN = 32;
void sb_check_w(const Tensor& t, int rows, int C, const char* what) {
  TORCH_CHECK(t.is_contiguous() && t.dim() == 2 && t.size(0) == rows && t.size(1) == C &&
                  t.scalar_type() == torch::kBFloat16 && (reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0,
              "sample block: ", what, " must be a contiguous 16-byte aligned bf16 (", rows, ", ", C, ") weight");
}
void sb_check_v(const Tensor& t, int n, const char* what) {
  TORCH_CHECK(t.is_contiguous() && t.numel() == n && t.scalar_type() == torch::kFloat32 &&
                  (reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0,
              "sample block: ", what, " must be a contiguous 16-byte aligned fp32 vector of ", n);
}
// per layer the 12 parameters in layer_spec_and_params order with the bf16 weight shadows:
// (g1, be1, wqkv_bf16, bqkv, wo_bf16, bo, g2, be2, w1_bf16, b1, w2_bf16, b2)
void sb_fill_params(pio::SBLayer& y, const std::vector<Tensor>& p, int i, int C) {
  const Tensor* q = &p[12 * i];
  sb_check_v(q[0], C, "γ1"); sb_check_v(q[1], C, "β1"); sb_check_w(q[2], 3 * C, C, "Wqkv");
  sb_check_v(q[3], 3 * C, "bqkv"); sb_check_w(q[4], C, C, "Wo"); sb_check_v(q[5], C, "bo");
  sb_check_v(q[6], C, "γ2"); sb_check_v(q[7], C, "β2"); sb_check_w(q[8], C, C, "W1");
  sb_check_v(q[9], C, "b1"); sb_check_w(q[10], C, C, "W2"); sb_check_v(q[11], C, "b2");
  y.g1 = f32p(q[0]); y.be1 = f32p(q[1]); y.Wqkv = bfp(q[2]); y.bqkv = f32p(q[3]); y.Wo = bfp(q[4]); y.bo = f32p(q[5]);
  y.g2 = f32p(q[6]); y.be2 = f32p(q[7]); y.W1 = bfp(q[8]); y.b1 = f32p(q[9]); y.W2 = bfp(q[10]); y.b2 = f32p(q[11]);
}
constexpr int kSBSaved = 12;  // LN1X QKV O LN2Y U GU Y Z mean1 rstd1 mean2 rstd2
void sb_fill_saved(pio::SBLayer& y, const std::vector<Tensor>& sv, int i, int R, int C) {
  const Tensor* t = &sv[kSBSaved * i];
  for (int k = 0; k < kSBSaved; ++k) {
    const int64_t want = k < 8 ? (int64_t)R * (k == 1 ? 3 * C : C) : R;
    TORCH_CHECK(t[k].is_contiguous() && t[k].numel() == want &&
                    t[k].scalar_type() == (k < 6 ? torch::kBFloat16 : torch::kFloat32),
                "sample block: saved tensor ", k, " of layer ", i, " has the wrong shape / dtype");
  }
  y.LN1X = reinterpret_cast<uint16_t*>(t[0].data_ptr()); y.QKV = reinterpret_cast<uint16_t*>(t[1].data_ptr());
  y.O = reinterpret_cast<uint16_t*>(t[2].data_ptr()); y.LN2Y = reinterpret_cast<uint16_t*>(t[3].data_ptr());
  y.U = reinterpret_cast<uint16_t*>(t[4].data_ptr()); y.GU = reinterpret_cast<uint16_t*>(t[5].data_ptr());
  y.Y = t[6].data_ptr<float>(); y.Z = t[7].data_ptr<float>(); y.mean1 = t[8].data_ptr<float>();
  y.rstd1 = t[9].data_ptr<float>(); y.mean2 = t[10].data_ptr<float>(); y.rstd2 = t[11].data_ptr<float>();
}
}  // namespace

// the pre stage's 10 tensors: [O (R, C) bf16, x_q (R, C) or (32, C) fp32, wo_bf16, bo, g2, be2,
// w1_bf16, b1, w2_bf16, b2]
namespace {
void sb_fill_pre(pio::SBLayer& y, const std::vector<Tensor>& pre, int C) {
  sb_check_w(pre[2], C, C, "pre Wo"); sb_check_v(pre[3], C, "pre bo"); sb_check_v(pre[4], C, "pre γ2");
  sb_check_v(pre[5], C, "pre β2"); sb_check_w(pre[6], C, C, "pre W1"); sb_check_v(pre[7], C, "pre b1");
  sb_check_w(pre[8], C, C, "pre W2"); sb_check_v(pre[9], C, "pre b2");
  y.Wo = bfp(pre[2]); y.bo = f32p(pre[3]); y.g2 = f32p(pre[4]); y.be2 = f32p(pre[5]);
  y.W1 = bfp(pre[6]); y.b1 = f32p(pre[7]); y.W2 = bfp(pre[8]); y.b2 = f32p(pre[9]);
}
constexpr int kSBPreSaved = 6;  // LN2Y U GU (bf16) Y mean2 rstd2 (fp32)
void sb_fill_pre_saved(pio::SBLayer& y, const std::vector<Tensor>& sv, int R, int C) {
  TORCH_CHECK((int)sv.size() == kSBPreSaved, "sample block: 6 saved pre-stage tensors");
  for (int k = 0; k < kSBPreSaved; ++k) {
    const int64_t want = k < 4 ? (int64_t)R * C : R;
    TORCH_CHECK(sv[k].is_contiguous() && sv[k].numel() == want &&
                    sv[k].scalar_type() == (k < 3 ? torch::kBFloat16 : torch::kFloat32),
                "sample block: saved pre-stage tensor ", k, " has the wrong shape / dtype");
  }
  y.LN2Y = reinterpret_cast<uint16_t*>(sv[0].data_ptr()); y.U = reinterpret_cast<uint16_t*>(sv[1].data_ptr());
  y.GU = reinterpret_cast<uint16_t*>(sv[2].data_ptr()); y.Y = sv[3].data_ptr<float>();
  y.mean2 = sv[4].data_ptr<float>(); y.rstd2 = sv[5].data_ptr<float>();
}
void sb_check_pre_o(const Tensor& o, int R, int C) {
  TORCH_CHECK(o.is_contiguous() && o.dim() == 2 && o.size(0) == R && o.size(1) == C && o.scalar_type() == torch::kBFloat16 &&
                  (reinterpret_cast<uintptr_t>(o.data_ptr()) & 15) == 0,
              "sample block: pre O must be (B·32, C) contiguous bf16");
}
}  // namespace

// forward of a whole block, one workgroup per sample: x (B·32, C) fp32 → per layer
// [LN1X, QKV, O, LN2Y, U, GU (bf16), Y, Z, mean1, rstd1, mean2, rstd2 (fp32)]; the block output is
// the last layer's Z.  pre (10 tensors, see sb_fill_pre): the cross layer's post-attention half
// runs first and WRITES x (its output, the block input); its 6 saved tensors are appended.
// post (4 tensors [γq, βq, wq_bf16 (C, C), bq]): the next cross layer's LN + query projection of the
// block output; [Q (R, C) bf16, LN_q(z) (R, C) bf16, mean, rstd] are appended (after pre's)
namespace {
void sb_fill_post(pio::SBQPath& q, const std::vector<Tensor>& post, int C) {
  TORCH_CHECK(post.size() == 4, "sample block: post = [γ, β, w (N, C) bf16, bias (N)], N ∈ {C, 2C}");
  const int N = post[2].dim() == 2 ? (int)post[2].size(0) : 0;
  TORCH_CHECK(N == C || N == 2 * C, "sample block: the post projection has C or 2C outputs");
  sb_check_v(post[0], C, "post γ"); sb_check_v(post[1], C, "post β"); sb_check_w(post[2], N, C, "post W");
  sb_check_v(post[3], N, "post bias");
  q.N = N; q.g = f32p(post[0]); q.b = f32p(post[1]); q.Wq = bfp(post[2]); q.bq = f32p(post[3]);
}
}  // namespace

std::vector<Tensor> sb_fwd(Tensor x, std::vector<Tensor> params, double scale, double eps, std::vector<Tensor> pre,
                           std::vector<Tensor> post) {
  const int C = x.dim() == 2 ? (int)x.size(1) : 0;
  TORCH_CHECK(x.is_contiguous() && (C == 64 || C == 128) && x.size(0) % kSBN == 0 && x.size(0) > 0,
              "sb_fwd: x (B·32, C), C ∈ {64, 128}");
  CHECK_DT(x, torch::kFloat32);
  const int L = (int)params.size() / 12, R = (int)x.size(0);
  TORCH_CHECK(L >= 1 && L <= pio::kSBMaxLayers && (int)params.size() == 12 * L, "sb_fwd: 1..4 layers × 12 parameters");
  auto f32 = x.options().dtype(torch::kFloat32);
  auto b16 = x.options().dtype(torch::kBFloat16);
  pio::SBFwdArgs a{};
  a.X0 = f32p(x); a.L = L; a.B = R / kSBN;
  a.scale_log2 = (float)(scale * 1.4426950408889634);
  a.eps = (float)eps;
  std::vector<Tensor> out;
  for (int i = 0; i < L; ++i) {
    sb_fill_params(a.ly[i], params, i, C);
    std::vector<Tensor> sv{torch::empty({R, C}, b16), torch::empty({R, 3 * C}, b16), torch::empty({R, C}, b16),
                           torch::empty({R, C}, b16), torch::empty({R, C}, b16), torch::empty({R, C}, b16),
                           torch::empty({R, C}, f32), torch::empty({R, C}, f32), torch::empty({R}, f32),
                           torch::empty({R}, f32), torch::empty({R}, f32), torch::empty({R}, f32)};
    out.insert(out.end(), sv.begin(), sv.end());
    sb_fill_saved(a.ly[i], out, i, R, C);
  }
  if (!pre.empty()) {
    TORCH_CHECK(pre.size() == 10, "sb_fwd: pre = [O, x_q, wo, bo, g2, be2, w1, b1, w2, b2]");
    sb_check_pre_o(pre[0], R, C);
    const Tensor& xq = pre[1];
    TORCH_CHECK(xq.is_contiguous() && xq.dim() == 2 && xq.size(1) == C && (xq.size(0) == R || xq.size(0) == kSBN) &&
                    xq.scalar_type() == torch::kFloat32,
                "sb_fwd: pre x_q must be (B·32, C) or broadcast (32, C) fp32");
    sb_fill_pre(a.pre, pre, C);
    std::vector<Tensor> sv{torch::empty({R, C}, b16), torch::empty({R, C}, b16), torch::empty({R, C}, b16),
                           torch::empty({R, C}, f32), torch::empty({R}, f32), torch::empty({R}, f32)};
    sb_fill_pre_saved(a.pre, sv, R, C);
    a.pre.Z = x.data_ptr<float>();
    a.preO = bfp(pre[0]);
    a.preX = f32p(xq);
    a.preX_bs = xq.size(0) == R ? kSBN : 0;
    a.has_pre = 1;
    out.insert(out.end(), sv.begin(), sv.end());
  }
  if (!post.empty()) {
    sb_fill_post(a.post, post, C);
    Tensor q = torch::empty({R, (int64_t)a.post.N}, b16), lnx = torch::empty({R, C}, b16), mean = torch::empty({R}, f32),
           rstd = torch::empty({R}, f32);
    a.post.Q = reinterpret_cast<uint16_t*>(q.data_ptr()); a.post.LNX = reinterpret_cast<uint16_t*>(lnx.data_ptr());
    a.post.mean = mean.data_ptr<float>(); a.post.rstd = rstd.data_ptr<float>();
    a.has_post = 1;
    out.insert(out.end(), {q, lnx, mean, rstd});
  }
  TORCH_CHECK(pio::sb_fwd_launch(a, C, stream()), "sb_fwd: launch refused");
  return out;
}

// backward of a block: dz (B·32, C) fp32, x0 the block input, saved = sb_fwd's outputs, params
// as sb_fwd's.  Returns [dx, the (B, 4·L·C) fp32 LayerNorm partial slab (row b: sample b's
// [dγ1 | dβ1 | dγ2 | dβ2] of layer 0, then layer 1, …; sum the rows into the gradients), then per
// layer the gradient rows dQKV, dY, dU, dZ (bf16)] for sb_wgrad
// pre (as sb_fwd's, x_q unused) + pre_saved (sb_fwd's 6 appended tensors): the cross layer's
// post-attention backward runs last; dx is then the gradient of its residual input x_q, and
// [dO (R, C) bf16, δ (R, 4) fp32, dY, dU, dZ (bf16 rows)] are appended; the LayerNorm slab rows
// are 2C wider (the pre stage's dγ2 | dβ2 last).  zero_out: an fp32 buffer of 4k elements the
// kernel clears (the cross attention backward's accumulators)
// post (as sb_fwd's) + post_io [dQ (R, C) fp32, dres (R, C) fp32, mean, rstd (sb_fwd's)]: the query
// path's backward runs first, dz is then unused; [dQ bf16 rows] is appended, the slab rows 2C wider
std::vector<Tensor> sb_bwd(Tensor dz, Tensor x0, std::vector<Tensor> saved, std::vector<Tensor> params, double scale,
                           double eps, std::vector<Tensor> pre, std::vector<Tensor> pre_saved, OptT zero_out,
                           std::vector<Tensor> post, std::vector<Tensor> post_io) {
  const int C = x0.dim() == 2 ? (int)x0.size(1) : 0;
  TORCH_CHECK(dz.is_contiguous() && x0.is_contiguous() && dz.sizes() == x0.sizes() && (C == 64 || C == 128) &&
                  x0.size(0) % kSBN == 0 && x0.size(0) > 0,
              "sb_bwd: dz / x0 (B·32, C), C ∈ {64, 128}");
  CHECK_DT(dz, torch::kFloat32);
  CHECK_DT(x0, torch::kFloat32);
  const int L = (int)params.size() / 12, R = (int)x0.size(0);
  TORCH_CHECK(L >= 1 && L <= pio::kSBMaxLayers && (int)params.size() == 12 * L && (int)saved.size() == kSBSaved * L,
              "sb_bwd: saved per layer");
  auto f32 = x0.options().dtype(torch::kFloat32);
  auto b16 = x0.options().dtype(torch::kBFloat16);
  pio::SBBwdArgs a{};
  a.X0 = f32p(x0); a.dZ = f32p(dz); a.L = L; a.B = R / kSBN;
  a.scale_log2 = (float)(scale * 1.4426950408889634);
  a.eps = (float)eps;
  Tensor dx = torch::empty({R, C}, f32);
  a.dX = dx.data_ptr<float>();
  const bool hp = !pre.empty(), hq = !post.empty();
  a.ln_rs = 4 * L * C + (hp ? 2 * C : 0) + (hq ? 2 * C : 0);
  Tensor lns = torch::empty({(int64_t)a.B, (int64_t)a.ln_rs}, f32);  // every element stored by the kernel
  std::vector<Tensor> out{dx, lns};
  for (int i = 0; i < L; ++i) {
    sb_fill_params(a.ly[i], params, i, C);
    sb_fill_saved(a.ly[i], saved, i, R, C);
    pio::SBGrad& g = a.gr[i];
    Tensor dq = torch::empty({R, 3 * C}, b16), dy = torch::empty({R, C}, b16), du = torch::empty({R, C}, b16),
           dzz = torch::empty({R, C}, b16);
    g.dQKV = reinterpret_cast<uint16_t*>(dq.data_ptr()); g.dY = reinterpret_cast<uint16_t*>(dy.data_ptr());
    g.dU = reinterpret_cast<uint16_t*>(du.data_ptr()); g.dZ = reinterpret_cast<uint16_t*>(dzz.data_ptr());
    float* lp = lns.data_ptr<float>() + (int64_t)4 * i * C;
    g.dg1 = lp; g.dbe1 = lp + C; g.dg2 = lp + 2 * C; g.dbe2 = lp + 3 * C;
    out.insert(out.end(), {dq, dy, du, dzz});
  }
  if (hp) {
    TORCH_CHECK(pre.size() == 10, "sb_bwd: pre = [O, x_q, wo, bo, g2, be2, w1, b1, w2, b2]");
    sb_check_pre_o(pre[0], R, C);
    sb_fill_pre(a.pre, pre, C);
    sb_fill_pre_saved(a.pre, pre_saved, R, C);
    a.pre.O = reinterpret_cast<uint16_t*>(pre[0].data_ptr());
    Tensor dO = torch::empty({R, C}, b16), delta = torch::empty({R, 4}, f32), dy = torch::empty({R, C}, b16),
           du = torch::empty({R, C}, b16), dzz = torch::empty({R, C}, b16);
    a.preDO = reinterpret_cast<uint16_t*>(dO.data_ptr());
    a.preDelta = delta.data_ptr<float>();
    pio::SBGrad& g = a.pgr;
    g.dY = reinterpret_cast<uint16_t*>(dy.data_ptr()); g.dU = reinterpret_cast<uint16_t*>(du.data_ptr());
    g.dZ = reinterpret_cast<uint16_t*>(dzz.data_ptr());
    float* lp = lns.data_ptr<float>() + (int64_t)4 * L * C;
    g.dg2 = lp; g.dbe2 = lp + C;
    a.has_pre = 1;
    out.insert(out.end(), {dO, delta, dy, du, dzz});
  }
  if (hq) {
    sb_fill_post(a.post, post, C);
    TORCH_CHECK(post_io.size() == 4, "sb_bwd: post_io = [dQ, dres (or empty), mean, rstd]");
    const bool has_dres = post_io[1].numel() > 0;
    for (int k = 0; k < 4; ++k) {
      if (k == 1 && !has_dres) continue;
      const int64_t want = k == 0 ? (int64_t)R * a.post.N : (k == 1 ? (int64_t)R * C : R);
      CHECK_DT(post_io[k], torch::kFloat32);
      TORCH_CHECK(post_io[k].is_contiguous() && post_io[k].numel() == want &&
                      (reinterpret_cast<uintptr_t>(post_io[k].data_ptr()) & 15) == 0,
                  "sb_bwd: post_io tensor ", k, " must be contiguous fp32 (R, N) / (R, C) / (R)");
    }
    a.post.dQ = f32p(post_io[0]); a.post.dres = has_dres ? f32p(post_io[1]) : nullptr;
    a.post.mean = post_io[2].data_ptr<float>(); a.post.rstd = post_io[3].data_ptr<float>();
    Tensor dqb = torch::empty({R, (int64_t)a.post.N}, b16);
    a.post.dQb = reinterpret_cast<uint16_t*>(dqb.data_ptr());
    float* lp = lns.data_ptr<float>() + (int64_t)(4 * L + (hp ? 2 : 0)) * C;
    a.post.dg = lp; a.post.db = lp + C;
    a.has_post = 1;
    out.push_back(dqb);
  }
  if (zero_out.has_value()) {
    CHECK_DT(*zero_out, torch::kFloat32);
    TORCH_CHECK(zero_out->is_contiguous() && zero_out->numel() % 4 == 0 &&
                    reinterpret_cast<uintptr_t>(zero_out->data_ptr()) % 16 == 0,
                "sb_bwd: zero_out must be a contiguous, 16-byte aligned fp32 buffer of 4k elements");
    a.zero_p = zero_out->data_ptr<float>();
    a.zero_n4 = zero_out->numel() / 4;
  }
  TORCH_CHECK(pio::sb_bwd_launch(a, C, stream()), "sb_bwd: launch refused");
  return out;
}

// grouped weight gradients of a block: jobs = [G (R, N) bf16, A (R, C) bf16, dW (N, C) fp32,
// db (N) fp32] × n (added to dW / db); one C for every job.  job_slab / job_dsts / job_offs: a
// slab reduction run by appended workgroups (the block's LayerNorm partials from sb_bwd)
void sb_wgrad(std::vector<Tensor> jobs, OptT job_slab, std::vector<Tensor> job_dsts, std::vector<int64_t> job_offs) {
  TORCH_CHECK(jobs.size() % 4 == 0 && !jobs.empty() && (int)jobs.size() / 4 <= pio::kSBMaxJobs, "sb_wgrad: 1..", pio::kSBMaxJobs, " jobs");
  pio::SBWgradArgs a{};
  a.njobs = (int)jobs.size() / 4;
  a.R = (int)jobs[0].size(0);
  const int C = jobs[1].dim() == 2 ? (int)jobs[1].size(1) : 0;
  TORCH_CHECK(C == 64 || C == 128, "sb_wgrad: A (R, C), C ∈ {64, 128}");
  for (int j = 0; j < a.njobs; ++j) {
    const Tensor &G = jobs[4 * j], &A = jobs[4 * j + 1], &dW = jobs[4 * j + 2], &db = jobs[4 * j + 3];
    const int N = (int)G.size(1);
    TORCH_CHECK(G.is_contiguous() && A.is_contiguous() && G.dim() == 2 && A.dim() == 2 && G.size(0) == a.R &&
                    A.size(0) == a.R && A.size(1) == C && G.scalar_type() == torch::kBFloat16 &&
                    A.scalar_type() == torch::kBFloat16 && N % 64 == 0 && N > 0,
                "sb_wgrad: G (R, N) / A (R, C) bf16");
    TORCH_CHECK(dW.is_contiguous() && dW.numel() == (int64_t)N * C && db.is_contiguous() && db.numel() == N,
                "sb_wgrad: dW (N, C) / db (N)");
    CHECK_DT(dW, torch::kFloat32);
    CHECK_DT(db, torch::kFloat32);
    a.job[j] = pio::SBWgradJob{bfp(G), bfp(A), dW.data_ptr<float>(), db.data_ptr<float>(), N, 0};
  }
  TORCH_CHECK(pio::sb_wgrad_launch(a, C, make_job(job_slab, job_dsts, job_offs), stream()), "sb_wgrad: launch refused");
}

// workgroups of a non-deterministic SlabJob (128 measured best on the MLM step: 96–128 ≈ equal,
// 192 and 256 slower: profiles/r5_ab/README.md)
int slab_job_target() { return 128; }

// the backward entry points below ACCUMULATE parameter gradients into caller-provided fp32
// tensors (normally views of the flat gradient buffer) with device atomics: no partial slabs,
// no reduction pass, no autograd AccumulateGrad adds
namespace {
float* grad_target(Tensor& t, int64_t numel, const char* what) {
  TORCH_CHECK(t.is_contiguous() && t.numel() == numel, "bad gradient target ", what);
  CHECK_DT(t, torch::kFloat32);
  return t.data_ptr<float>();
}
constexpr int kGradReplicas = 8;
// gradient target: K contiguous floats (any shape), or an (8, K) replica view with unit inner
// stride whose row stride is shared by every target of the call (workgroup i adds into row
// i % 8).  A 2-D target counts as replicated only when it is (8, K) with K == its numel / 8.
// Slab mode (slab_rows > 0): every target is an (slab_rows, K) view of ONE (tiles, P) slab —
// workgroup i stores its partial into row i (no atomics; ops/fused.py reduces the slab).
float* vec_target(Tensor& t, int64_t K, const char* what, int& vrs, int64_t slab_rows = 0) {
  CHECK_DT(t, torch::kFloat32);
  if (slab_rows > 0) {
    TORCH_CHECK(t.dim() == 2 && t.size(0) == slab_rows && t.size(1) == K && t.stride(1) == 1,
                "slab target ", what, " must be a (tiles, K) view");
    TORCH_CHECK(vrs < 0 || vrs == (int)t.stride(0), "slab targets must share one row stride");
    vrs = (int)t.stride(0);
  } else if (t.dim() == 2 && t.size(0) == kGradReplicas && t.size(1) == K) {
    TORCH_CHECK(t.stride(1) == 1, "bad replicated target ", what);
    TORCH_CHECK(vrs < 0 || vrs == (int)t.stride(0), "replicated targets must share one row stride");
    vrs = (int)t.stride(0);
  } else {
    TORCH_CHECK(t.is_contiguous() && t.numel() == K, "bad gradient target ", what);
    TORCH_CHECK(vrs <= 0, "mixing replicated and plain vector targets");
    vrs = 0;
  }
  return t.data_ptr<float>();
}
// a slab reduction job: dsts[j] += Σ_rows slab[:, offs[j] : offs[j] + dsts[j].numel()]
// (slab (S, P) contiguous fp32, P and every offset multiples of 4, ≤ 8 segments)
pio::SlabJob make_job(const OptT& slab, std::vector<Tensor>& dsts, const std::vector<int64_t>& offs) {
  pio::SlabJob j{};
  if (!slab.has_value()) return j;
  const Tensor& t = *slab;
  CHECK_DT(t, torch::kFloat32);
  TORCH_CHECK(t.dim() == 2 && t.is_contiguous() && t.size(1) % 4 == 0, "slab must be (S, P), P % 4 == 0");
  TORCH_CHECK(dsts.size() == offs.size() && dsts.size() <= (size_t)pio::kMaxSlabSegs, "slab job: ≤ 16 segments");
  const int P = (int)t.size(1);
  for (size_t q = 0; q < dsts.size(); ++q) {
    Tensor& d = dsts[q];
    CHECK_DT(d, torch::kFloat32);
    TORCH_CHECK(d.is_contiguous() && d.device() == t.device(), "slab job: destinations must be contiguous");
    TORCH_CHECK(offs[q] % 4 == 0 && offs[q] >= 0 && offs[q] + d.numel() <= P, "slab job: bad segment");
    if (d.numel() == 0) continue;
    j.dst[j.n] = d.data_ptr<float>(); j.off[j.n] = (int)offs[q]; j.len[j.n] = (int)d.numel(); ++j.n;
  }
  if (j.n == 0 || t.size(0) == 0) return j;
  j.slab = t.data_ptr<float>();
  j.S = (int)t.size(0);
  j.P = P;
  j.det = g_det ? 1 : 0;
  if (g_det) {  // one workgroup per 256 columns, all rows (common.h slab_reduce_block)
    j.nbx = (P + 255) / 256;
    j.nblk = j.nbx;
  } else {  // 1024-column blocks × row splits: ≈ slab_job_target() workgroups, one round
    j.nbx = (P + pio::kSlabColsPerBlock - 1) / pio::kSlabColsPerBlock;
    int nsy = std::max(1, std::min(j.S, slab_job_target() / j.nbx));
    const int rb = (j.S + nsy - 1) / nsy;
    nsy = (j.S + rb - 1) / rb;
    j.nblk = j.nbx * nsy;
  }
  return j;
}

// zero_out (optional): an fp32 buffer the kernel carrying this job clears on the way (the NEXT
// kernel's atomic accumulator, e.g. the cross-attention dQ) — no separate fill launch
pio::SlabJob with_zero_span(pio::SlabJob job, const OptT& zero_out, const Tensor& like) {
  if (zero_out.has_value()) {
    CHECK_DT(*zero_out, torch::kFloat32);
    TORCH_CHECK(zero_out->is_contiguous() && zero_out->numel() % 4 == 0 && zero_out->get_device() == like.get_device() &&
                    reinterpret_cast<uintptr_t>(zero_out->data_ptr()) % 16 == 0,
                "zero_out must be a contiguous, 16-byte aligned fp32 buffer of 4k elements");
    job.zero_p = zero_out->data_ptr<float>();
    job.zero_n4 = zero_out->numel() / 4;
  }
  return job;
}
}  // namespace

// grads = [dWo, dbo, dg2, dbe2, dW1, db1, dW2, db2]; returns (dy, dO, delta)
// slab: targets are (ceil(R/64), ·) views of one slab (see vec_target), reduced by slab_reduce
std::vector<Tensor> post_attn_bwd(Tensor dz, Tensor y, Tensor m2, Tensor r2, Tensor u, Tensor o, Tensor wo, Tensor w1,
                                  Tensor w2, Tensor g2, Tensor be2, int64_t H, std::vector<Tensor> grads, bool slab,
                                  OptT job_slab, std::vector<Tensor> job_dsts, std::vector<int64_t> job_offs,
                                  OptT seed, int64_t site, double p, OptT zero_out) {
  TORCH_CHECK(dz.is_contiguous() && y.is_contiguous() && u.is_contiguous() && o.is_contiguous(),
              "post_attn_bwd operands must be contiguous (R, C)");
  const int R = (int)dz.size(0), C = (int)dz.size(1);
  TORCH_CHECK(C == 32 || C == 64 || C == 128, "post_attn supports C in {32, 64, 128}");
  TORCH_CHECK(H > 0 && C % H == 0, "heads must divide C");
  TORCH_CHECK(grads.size() == 8, "post_attn_bwd needs 8 gradient targets");
  TORCH_CHECK(!g_det || slab, "deterministic mode: post_attn_bwd parameter gradients need slab mode (R < 2^17 rows)");
  const int64_t CC = (int64_t)C * C;
  int vrs = -1;
  const int64_t sr = slab ? (R + 63) / 64 : 0;
  pio::PostAttnGrads pg{vec_target(grads[0], CC, "dWo", vrs, sr), vec_target(grads[1], C, "dbo", vrs, sr),
                        vec_target(grads[2], C, "dg2", vrs, sr), vec_target(grads[3], C, "dbe2", vrs, sr),
                        vec_target(grads[4], CC, "dW1", vrs, sr), vec_target(grads[5], C, "db1", vrs, sr),
                        vec_target(grads[6], CC, "dW2", vrs, sr), vec_target(grads[7], C, "db2", vrs, sr), 0, 0};
  pg.vrs = vrs < 0 ? 0 : vrs;
  pg.slab = slab ? 1 : 0;
  auto f32 = dz.options().dtype(torch::kFloat32);
  Tensor dy = torch::empty({R, C}, f32);
  Tensor dO = torch::empty({R, C}, dz.options().dtype(torch::kBFloat16));
  Tensor delta = torch::empty({R, H}, f32);
  pio::PostAttnBwdArgs a{};
  a.dZ = f32p(dz);
  a.s.Ysave = f32p_mut(y);
  a.s.mean2 = f32p_mut(m2);
  a.s.rstd2 = f32p_mut(r2);
  a.s.Usave = bfp_mut(u);
  a.O = bfp(o);
  a.p.Wo = bfp(wo);
  a.p.W1 = bfp(w1);
  a.p.W2 = bfp(w2);
  a.p.g2 = f32p(g2);
  a.p.be2 = f32p(be2);
  a.dY = dy.data_ptr<float>();
  a.dO = bfp_mut(dO);
  a.delta = delta.data_ptr<float>();
  a.H = (int)H;
  a.grads = pg;
  a.R = R;
  a.job = with_zero_span(make_job(job_slab, job_dsts, job_offs), zero_out, dz);
  a.dr = make_drop(seed, site, p);
  pio::post_attn_bwd_launch(a, C, stream());
  return {dy, dO, delta};
}

// self-attention layer boundary l+1 → l, backward, slab mode only: the LN1+QKV backward of
// layer l+1 (g = dQKV (R, 3C) fp32, dres = dY_{l+1}) produces dZ_l in registers, the
// post-attention backward of layer l consumes it.  ll_grads = slab views for (dγ1, dβ1, dWqkv,
// dbqkv) of layer l+1, pa_grads = the 8 post-attention slab views of layer l — all of ONE slab.
// Returns (dy, dO, delta) of layer l.
std::vector<Tensor> ln_linear_post_attn_bwd(Tensor g, Tensor wq, Tensor x, Tensor mean1, Tensor rstd1, Tensor lnw,
                                            Tensor lnb, Tensor dres, std::vector<Tensor> ll_grads, Tensor y, Tensor m2,
                                            Tensor r2, Tensor u, Tensor o, Tensor wo, Tensor w1, Tensor w2, Tensor g2,
                                            Tensor be2, int64_t H, std::vector<Tensor> pa_grads, OptT job_slab,
                                            std::vector<Tensor> job_dsts, std::vector<int64_t> job_offs, OptT seed,
                                            int64_t site, double p, OptT zero_out, OptT att_qkv, OptT att_lse,
                                            OptT att_out, double att_scale) {
  TORCH_CHECK(y.is_contiguous() && u.is_contiguous() && o.is_contiguous() && x.is_contiguous() && dres.is_contiguous(),
              "operands must be contiguous (R, C)");
  const int R = (int)y.size(0), C = (int)y.size(1);
  TORCH_CHECK(C == 32 || C == 64 || C == 128, "the fused self-attention backward supports C in {32, 64, 128}");
  TORCH_CHECK(H > 0 && C % H == 0, "heads must divide C");
  const int nq = (int)wq.size(0);  // 3C: packed QKV of a self-attention layer; C: a cross-attention query projection
  TORCH_CHECK(wq.is_contiguous() && (nq == 3 * C || nq == C) && wq.size(1) == C, "wq must be (3C, C) or (C, C)");
  TORCH_CHECK(g.is_contiguous() && g.size(0) == R && g.size(1) == nq, "g must be (R, rows(wq)) contiguous");
  TORCH_CHECK(g.scalar_type() == torch::kFloat32 || g.scalar_type() == torch::kBFloat16, "g must be fp32 or bf16");
  TORCH_CHECK(x.size(0) == R && x.size(1) == C && dres.size(0) == R && dres.size(1) == C, "x / dres must be (R, C)");
  TORCH_CHECK(ll_grads.size() == 4 && pa_grads.size() == 8, "4 + 8 slab targets expected");
  const int64_t sr = (R + 63) / 64, CC = (int64_t)C * C;
  int vrs = -1;
  auto T = [&](Tensor& t, int64_t K, const char* what) { return vec_target(t, K, what, vrs, sr); };
  float* dg1 = T(ll_grads[0], C, "dlnw");
  float* db1 = T(ll_grads[1], C, "dlnb");
  float* dwq = T(ll_grads[2], (int64_t)nq * C, "dWqkv");
  float* dbq = T(ll_grads[3], nq, "dbqkv");
  pio::PostAttnGrads pg{T(pa_grads[0], CC, "dWo"), T(pa_grads[1], C, "dbo"), T(pa_grads[2], C, "dg2"),
                        T(pa_grads[3], C, "dbe2"), T(pa_grads[4], CC, "dW1"), T(pa_grads[5], C, "db1"),
                        T(pa_grads[6], CC, "dW2"), T(pa_grads[7], C, "db2"), vrs, 1};
  auto f32 = y.options().dtype(torch::kFloat32);
  Tensor dy = torch::empty({R, C}, f32);
  Tensor dO = torch::empty({R, C}, y.options().dtype(torch::kBFloat16));
  Tensor delta = torch::empty({R, H}, f32);
  pio::LnLinearPostAttnBwdArgs a{};
  a.next.Wq = bfp(wq);
  a.next.lnw = f32p(lnw);
  a.next.lnb = f32p(lnb);
  a.next.mean1 = f32p_mut(mean1);
  a.next.rstd1 = f32p_mut(rstd1);
  a.next.nq = nq;
  a.X = f32p(x);
  a.dres = f32p(dres);
  a.dlnw = dg1;
  a.dlnb = db1;
  a.dWq = dwq;
  a.dbq = dbq;
  a.pa.s.Ysave = f32p_mut(y);
  a.pa.s.mean2 = f32p_mut(m2);
  a.pa.s.rstd2 = f32p_mut(r2);
  a.pa.s.Usave = bfp_mut(u);
  a.pa.O = bfp(o);
  a.pa.p.Wo = bfp(wo);
  a.pa.p.W1 = bfp(w1);
  a.pa.p.W2 = bfp(w2);
  a.pa.p.g2 = f32p(g2);
  a.pa.p.be2 = f32p(be2);
  a.pa.dY = dy.data_ptr<float>();
  a.pa.dO = bfp_mut(dO);
  a.pa.delta = delta.data_ptr<float>();
  a.pa.H = (int)H;
  a.pa.grads = pg;
  a.pa.R = R;
  a.pa.job = with_zero_span(make_job(job_slab, job_dsts, job_offs), zero_out, y);
  a.pa.dr = make_drop(seed, site, p);
  // att_*: the layer below's attention backward fused in (N = 64 latents per sample, the tile is
  // the sample): its packed QKV rows and LSE in, its dQKV (R, 3C) bf16 out; dO / delta are then
  // not produced (the returned tensors are unwritten)
  if (att_out.has_value()) {
    TORCH_CHECK(att_qkv.has_value() && att_lse.has_value(), "att_out needs att_qkv and att_lse");
    CHECK_DT(*att_qkv, torch::kBFloat16); CHECK_DT(*att_out, torch::kBFloat16); CHECK_DT(*att_lse, torch::kFloat32);
    TORCH_CHECK(C == 64 && H == 4 && R % 64 == 0, "fused attention backward: C = 64, H = 4, R % 64 == 0");
    TORCH_CHECK(att_qkv->is_contiguous() && att_qkv->numel() == (int64_t)R * 3 * C && att_out->is_contiguous() &&
                    att_out->numel() == (int64_t)R * 3 * C && att_lse->is_contiguous() && att_lse->numel() == (int64_t)R * H,
                "fused attention backward: qkv / out (R, 3C), lse (R, H) contiguous");
    a.att.qkv = bfp(*att_qkv);
    a.att.lse = f32p(*att_lse);
    a.att.out = bfp_mut(*att_out);
  }
  a.att.scale = (float)att_scale;
  auto launch = [&](const Tensor& gg) {
    a.G = gg.data_ptr();
    a.g_bf16 = gg.scalar_type() == torch::kBFloat16;
    return pio::ln_linear_post_attn_bwd_launch(a, C, stream());
  };
  // a bf16 G (from attn_bwd's bf16 outputs) is taken by the chain-layout kernel; any other
  // kernel gets it widened to fp32 (same values)
  if (!launch(g)) TORCH_CHECK(!a.att.out && launch(g.to(torch::kFloat32)), "ln_linear_post_attn_bwd: launch failed");
  return {dy, dO, delta};
}

// dX = LN_bwd(g·w) (+ dres); accumulates dγ/dβ (dlnw/dlnb, needed when lnw is given) and, when
// dW is given, dW += gᵀ·LN(x) and db += Σ_rows g.  Returns dX when need_dx.
constexpr int kTallRows = 1 << 17;

OptT ln_linear_bwd(Tensor g, Tensor w, Tensor x, OptT mean, OptT rstd, OptT lnw, OptT lnb, OptT dres, bool need_dx,
                   OptT dlnw, OptT dlnb, OptT dW, OptT db, OptT pe, int64_t kin, bool slab, OptT job_slab,
                   std::vector<Tensor> job_dsts, std::vector<int64_t> job_offs, OptT dx_out, OptT pe_index) {
  TORCH_CHECK(g.dim() == 2 && g.stride(1) == 1 && x.dim() == 2 && x.stride(1) == 1, "g / x must be 2-D rows");
  const int R = (int)g.size(0), N = (int)g.size(1);
  TORCH_CHECK(!(slab && R >= kTallRows), "slab gradients are for R < ", kTallRows, " rows");
  TORCH_CHECK(!g_det || slab || (!dW.has_value() && !lnw.has_value()),
              "deterministic mode: ln_linear_bwd parameter gradients need slab mode (R < 2^17 rows)");
  const int64_t sr = slab ? (R + 63) / 64 : 0;
  const int Kin = kin >= 0 ? (int)kin : (int)w.size(1);
  TORCH_CHECK(w.size(0) == N && w.is_contiguous() && w.size(1) >= Kin, "w must be (N, >= Kin) contiguous, N = g columns");
  TORCH_CHECK(x.size(0) == R && (pe.has_value() || x.size(1) == Kin), "x must be (R, Kin)");
  TORCH_CHECK(!(pe.has_value() && need_dx), "no input gradient for a split (pixels + PE) input");
  const pio::PeSplit ps = pe_split(pe, x, R, Kin, pe_index);
  TORCH_CHECK(Kin <= 160, "ln_linear_bwd supports Kin <= 160");
  auto f32 = g.options().dtype(torch::kFloat32);
  Tensor dx;
  float *dxp = nullptr, *dgp = nullptr, *dbp = nullptr, *dwp = nullptr, *dbiasp = nullptr;
  int vrs = -1;
  int dx_rs = Kin;
  if (need_dx && dx_out.has_value()) {
    // dX into a given (R, Kin) fp32 buffer (e.g. a parameter's gradient view); it may BE dres
    // (read and written element-wise by the same thread: dX = LN_bwd(...) + dres in place)
    CHECK_DT(*dx_out, torch::kFloat32);
    TORCH_CHECK(dx_out->dim() == 2 && dx_out->size(0) == R && dx_out->size(1) == Kin && dx_out->stride(1) == 1,
                "dx_out must be (R, Kin) rows");
    TORCH_CHECK(!dres.has_value() || dres->data_ptr() != dx_out->data_ptr() || dres->stride(0) == dx_out->stride(0),
                "dx_out aliasing dres needs the same row stride");
    dx = *dx_out; dxp = dx.data_ptr<float>(); dx_rs = (int)dx.stride(0);
  } else if (need_dx) { dx = torch::empty({R, Kin}, f32); dxp = dx.data_ptr<float>(); }
  if (lnw.has_value()) {
    TORCH_CHECK(lnb.has_value() && mean.has_value() && rstd.has_value(), "LN weight needs bias and row stats");
    TORCH_CHECK(dlnw.has_value() && dlnb.has_value(), "LN grad targets required");
    dgp = vec_target(*dlnw, Kin, "dlnw", vrs, sr);
    dbp = vec_target(*dlnb, Kin, "dlnb", vrs, sr);
  }
  int wrs = -1;  // the weight target's replica stride may differ from the vectors'
  if (dW.has_value()) dwp = vec_target(*dW, (int64_t)N * Kin, "dW", wrs, sr);
  if (db.has_value()) { TORCH_CHECK(dW.has_value(), "db needs dW"); dbiasp = vec_target(*db, N, "db", vrs, sr); }
  TORCH_CHECK(!slab || vrs < 0 || wrs < 0 || vrs == wrs, "slab targets must share one slab");
  // very tall inputs (image K/V projections): the weight gradient leaves the row-tile kernel
  // for the streaming tall-wgrad kernel (one partial per ~R/128 rows instead of per 64)
  const bool tall = dwp != nullptr && R >= kTallRows;
  pio::LnLinearBwdArgs a{};
  a.G = rows_in(g);
  a.N = N;
  a.W = bfp(w);
  a.w_rs = (int)w.size(1);
  a.Kin = Kin;
  a.X = rows_in(x);
  a.mean = f32o(mean);
  a.rstd = f32o(rstd);
  a.lnw = f32o(lnw);
  a.lnb = f32o(lnb);
  if (dres.has_value()) { a.dres = f32p(*dres); a.dres_rs = (int)dres->stride(0); TORCH_CHECK(dres->stride(1) == 1); }
  a.dX = dxp;
  a.dx_rs = dx_rs;
  a.dlnw = dgp;
  a.dlnb = dbp;
  a.dW = tall ? nullptr : dwp;
  a.db = tall ? nullptr : dbiasp;
  a.vrs = vrs < 0 ? 0 : vrs;
  a.wrs = wrs < 0 ? 0 : wrs;
  a.slab = slab ? 1 : 0;
  a.R = R;
  a.ps = ps;
  a.job = make_job(job_slab, job_dsts, job_offs);
  pio::ln_linear_bwd_launch(a, stream());
  if (tall) {
    pio::WgradArgs wa{};
    wa.G = a.G;
    wa.N = N;
    wa.A = a.X;
    wa.Kin = Kin;
    wa.amode = lnw.has_value() ? 1 : 0;
    wa.mean = a.mean;
    wa.rstd = a.rstd;
    wa.lnw = a.lnw;
    wa.lnb = a.lnb;
    wa.R = R;
    wa.rows_per_wg = 0;
    wa.dW = dwp;
    wa.db = dbiasp;
    wa.vrs = a.vrs;
    wa.wrs = a.wrs;
    wa.ps = ps;
    pio::wgrad_launch(wa, stream());
  }
  if (need_dx) return dx;
  return c10::nullopt;
}

// dW (+)= gᵀ·A', db (+)= Σ rows g  (A' = a | LN(a) | GELU(a); a may be pixels with a PE table)
void wgrad(Tensor g, Tensor a, int64_t amode, OptT mean, OptT rstd, OptT lnw, OptT lnb, int64_t rows_per_wg, Tensor dW,
           OptT db, OptT pe, int64_t kin, OptT pe_index) {
  TORCH_CHECK(g.dim() == 2 && a.dim() == 2 && g.stride(1) == 1 && a.stride(1) == 1, "2-D row tensors expected");
  const int R = (int)g.size(0), N = (int)g.size(1);
  const int Kin = kin >= 0 ? (int)kin : (int)a.size(1);
  TORCH_CHECK(a.size(0) == R, "row mismatch");
  TORCH_CHECK(pe.has_value() || a.size(1) == Kin, "a must be (R, Kin)");
  TORCH_CHECK(Kin <= 160, "wgrad supports Kin <= 160");
  TORCH_CHECK(!g_det, "deterministic mode: the streaming wgrad kernel adds partials with atomics");
  TORCH_CHECK(amode != 1 || (mean.has_value() && rstd.has_value() && lnw.has_value() && lnb.has_value()),
              "LN mode needs stats and affine");
  pio::WgradArgs wa{};
  wa.ps = pe_split(pe, a, R, Kin, pe_index);
  int wrs = -1, vrs = -1;
  wa.dW = vec_target(dW, (int64_t)N * Kin, "dW", wrs);
  wa.db = db.has_value() ? vec_target(*db, N, "db", vrs) : nullptr;
  wa.vrs = vrs < 0 ? 0 : vrs;
  wa.wrs = wrs < 0 ? 0 : wrs;
  wa.G = rows_in(g);
  wa.N = N;
  wa.A = rows_in(a);
  wa.Kin = Kin;
  wa.amode = (int)amode;
  wa.mean = f32o(mean);
  wa.rstd = f32o(rstd);
  wa.lnw = f32o(lnw);
  wa.lnb = f32o(lnb);
  wa.R = R;
  wa.rows_per_wg = (int)rows_per_wg;
  pio::wgrad_launch(wa, stream());
}

// per-device ticket of the CE combine kernel (its last workgroup sums the per-block partials):
// zero between launches (reset by its last taker); calls on a device are stream-ordered.
// Allocated once, so captured graphs never see it move.
constexpr int64_t kCeTickets = 4;
static Tensor& ce_ticket(const Tensor& like) {
  static std::unordered_map<int, Tensor> tickets;
  const int d = like.get_device();
  auto it = tickets.find(d);
  if (it == tickets.end()) it = tickets.emplace(d, torch::zeros({kCeTickets}, like.options().dtype(torch::kInt32))).first;
  return it->second;
}
// per-row-block arrival counters of the two-pass head's forward (re-armed by the kernel itself)
constexpr int64_t kCeRowBlockTickets = 4096;
static Tensor& ce_rb_tickets(const Tensor& like) {
  static std::unordered_map<int, Tensor> tickets;
  const int d = like.get_device();
  auto it = tickets.find(d);
  if (it == tickets.end())
    it = tickets.emplace(d, torch::zeros({kCeRowBlockTickets}, like.options().dtype(torch::kInt32))).first;
  return it->second;
}

// labels (B, L) → [idx_b (B, cap), labels_b (B, cap), gidx (gcap), glabels (gcap), total (1) fp32,
// overflow (1) bool (+ q (B, cap, C) = queries[idx_b] when the output-query array is given)]:
// per-sequence slots of the selected positions and their global compaction, one launch.
// sticky: optional persistent bool the kernel sets when this call overflows (never clears)
std::vector<Tensor> mlm_select(Tensor labels, int64_t cap, int64_t gcap, OptT sticky, OptT queries) {
  CHECK_DT(labels, torch::kInt64);
  TORCH_CHECK(labels.dim() == 2 && labels.is_contiguous(), "labels must be (B, L) contiguous");
  const int B = (int)labels.size(0), L = (int)labels.size(1);
  TORCH_CHECK(cap > 0 && cap <= L && gcap > 0 && B > 0, "bad capacities");
  auto i64 = labels.options();
  Tensor idx_b = torch::empty({B, cap}, i64), lab_b = torch::empty({B, cap}, i64);
  Tensor count = torch::empty({B}, i64.dtype(torch::kInt32));
  Tensor gidx = torch::empty({gcap}, i64), glab = torch::empty({gcap}, i64);
  Tensor total = torch::empty({1}, i64.dtype(torch::kFloat32)), ovf = torch::empty({1}, i64.dtype(torch::kBool));
  const float* P = nullptr;
  float* qp = nullptr;
  int C = 0;
  Tensor q;
  if (queries.has_value()) {
    CHECK_DT(*queries, torch::kFloat32);
    TORCH_CHECK(queries->dim() == 2 && queries->is_contiguous() && queries->size(0) >= L && queries->size(1) % 4 == 0 &&
                    queries->get_device() == labels.get_device(),
                "mlm_select: queries must be a contiguous fp32 (>= L, C) array, C % 4 == 0, on the labels' device");
    C = (int)queries->size(1);
    P = queries->data_ptr<float>();
    q = torch::empty({B, cap, C}, queries->options());
    qp = q.data_ptr<float>();
  }
  pio::mlm_select_launch(labels.data_ptr<int64_t>(), B, L, (int)cap, (int)gcap, idx_b.data_ptr<int64_t>(),
                         lab_b.data_ptr<int64_t>(), count.data_ptr<int>(), gidx.data_ptr<int64_t>(),
                         glab.data_ptr<int64_t>(), total.data_ptr<float>(), ovf.data_ptr<bool>(),
                         sticky.has_value() ? sticky->data_ptr<bool>() : nullptr, P, C, qp, stream());
  std::vector<Tensor> out{idx_b, lab_b, gidx, glab, total, ovf};
  if (queries.has_value()) out.push_back(q);
  return out;
}

static const int64_t* opt_idx(const OptT& idx, int64_t n) {
  if (!idx.has_value()) return nullptr;
  CHECK_DT(*idx, torch::kInt64);
  TORCH_CHECK(idx->is_contiguous() && idx->numel() == n, "ce: idx must hold one source row per row");
  return idx->data_ptr<int64_t>();
}

// mean CE over the rows of h (fp32 (N, C); row r = h[idx[r]] when idx is given, else h[r]) with
// label ≥ 0: → {loss (0-dim) = Σ rows / max(count, 1), per-row lse (M,), the compact bf16 rows
// hs (M, C) the backward kernels read}.  count: fp32 (1,).
// zero_out: an optional fp32 buffer the kernel clears on the way (the backward's dH accumulator)
// count_labels: count is an OUTPUT — the combine kernel writes the number of rows with a label
// ≥ 0 into it (no framework compare + reduce kernels ahead of the head; the backward reads it)
std::vector<Tensor> ce_fwd(Tensor h, OptT idx, Tensor labels, Tensor w, Tensor bias, Tensor count, OptT zero_out,
                           bool count_labels) {
  TORCH_CHECK(h.is_contiguous() && w.is_contiguous() && labels.is_contiguous() && bias.is_contiguous());
  CHECK_DT(labels, torch::kInt64);
  CHECK_DT(h, torch::kFloat32);
  CHECK_DT(count, torch::kFloat32);
  pio::CeFwdArgs a{};
  const int M = a.M = (int)labels.numel(), C = a.C = (int)h.size(1);
  a.V = (int)w.size(0);
  TORCH_CHECK(w.size(1) == C && (C == 32 || C == 64 || C == 128), "bad vocab head shape");
  TORCH_CHECK(idx.has_value() || h.size(0) == M, "ce_fwd: h must have one row per label without idx");
  a.hidx = opt_idx(idx, M);
  // C = 64, the two-pass head (ce_head.hip): the forward also forms the per-split Σ_v p·W partials
  // of each row (the hidden-state gradient up to the row-loss scale once merged); returned with
  // the splits' (max, sum) as a 4th and 5th output for ce_bwd, which merges them
  const pio::CeFwdPlan pl = pio::ce_fwd_plan(C, M, a.V);
  TORCH_CHECK(pl.rb_tickets <= kCeRowBlockTickets, "ce_fwd: too many rows for the row-block tickets");
  TORCH_CHECK(count.numel() >= 1 && count.is_contiguous(), "ce_fwd: count must hold one fp32 value");
  if (zero_out.has_value()) {
    CHECK_DT(*zero_out, torch::kFloat32);
    TORCH_CHECK(zero_out->is_contiguous() && zero_out->numel() % 4 == 0 && zero_out->get_device() == h.get_device() &&
                    reinterpret_cast<uintptr_t>(zero_out->data_ptr()) % 16 == 0,
                "ce_fwd: zero_out must be a contiguous, 16-byte aligned fp32 buffer of 4k elements");
    a.zero_out = zero_out->data_ptr<float>();
    a.zero_n = zero_out->numel();
  }
  auto f32 = h.options().dtype(torch::kFloat32);
  Tensor pml = torch::empty({pl.nsplit, M, 2}, f32), pacc;
  if (pl.acc) pacc = torch::empty({pl.nsplit, M, C}, f32);
  Tensor picked = torch::empty({M}, f32), lse = torch::empty({M}, f32), loss = torch::empty({}, f32);
  Tensor blk = torch::empty({2 * pl.nblk}, f32);
  Tensor hs = torch::empty({M, C}, h.options().dtype(torch::kBFloat16));
  a.H = h.data_ptr<float>(); a.labels = labels.data_ptr<int64_t>(); a.W = bfp(w); a.bias = f32p(bias);
  a.loss = loss.data_ptr<float>(); a.lse = lse.data_ptr<float>(); a.hs = bfp_mut(hs);
  a.count = count.data_ptr<float>(); a.count_labels = count_labels ? 1 : 0;
  a.nsplit = pl.nsplit; a.part_ml = pml.data_ptr<float>(); a.part_acc = pl.acc ? pacc.data_ptr<float>() : nullptr;
  a.picked = picked.data_ptr<float>(); a.blk = blk.data_ptr<float>();
  a.ticket = reinterpret_cast<unsigned*>(ce_ticket(h).data_ptr<int>());
  a.rb_tickets = pl.rb_tickets ? reinterpret_cast<unsigned*>(ce_rb_tickets(h).data_ptr<int>()) : nullptr;
  pio::ce_fwd_launch(a, stream());
  checked_sync("ce_fwd");
  if (pl.acc) return {loss, lse, hs, pacc, pml};
  return {loss, lse, hs};
}

// h: the compact bf16 rows from ce_fwd.  dH (+)= rows: row r lands in dH[rowmap[r]] when rowmap
// is given (dH then has the full (positions, C) shape), else in dH[r]; dW / db accumulate or
// overwrite.  The row-loss gradient
// is gout / max(count, 1) (gout: the 0-dim gradient of the mean loss).
// slab: the dW kernel stores its row-split partials into a returned (splits, V·C + V₄) slab
// instead of adding them (the caller sums it into dW | db with a slab job, offsets 0 and V·C).
OptT ce_bwd(Tensor h, Tensor labels, Tensor w, Tensor bias, Tensor lse, Tensor gout, Tensor count, Tensor dH,
            Tensor dW, Tensor db, bool accumulate, OptT rowmap, bool slab, OptT u, OptT u_ml) {
  const int M = (int)labels.numel(), C = (int)h.size(1), V = (int)w.size(0);
  CHECK_DT(h, torch::kBFloat16);
  TORCH_CHECK(h.size(0) == M, "ce_bwd: h must be the compact (M, C) bf16 rows of ce_fwd");
  CHECK_DT(gout, torch::kFloat32);
  CHECK_DT(count, torch::kFloat32);
  TORCH_CHECK(h.is_contiguous() && dH.is_contiguous() && dW.is_contiguous() && db.is_contiguous());
  TORCH_CHECK(dH.dim() == 2 && dH.size(1) == C, "dH must be (rows, C)");
  const int64_t* rm = nullptr;
  if (rowmap.has_value()) {
    CHECK_DT(*rowmap, torch::kInt64);
    TORCH_CHECK(rowmap->is_contiguous() && rowmap->numel() == M, "rowmap must hold one row index per row");
    rm = rowmap->data_ptr<int64_t>();
  } else {
    TORCH_CHECK(dH.size(0) == M, "dH must be (M, C) without a rowmap");
  }
  TORCH_CHECK(C != 64 || (u.has_value() && u_ml.has_value()),
              "ce_bwd: the two-pass head (C = 64) needs u and u_ml, the split partials ce_fwd returns with it");
  pio::CeBwdArgs a{};
  if (u.has_value()) {  // the two-pass head's backward: dW / db pass + the dH rows g·u
    // u: the forward's per-split Σ p·W partials (splits, M, 64), u_ml: their (max, sum) (splits, M, 2)
    CHECK_DT(*u, torch::kFloat32);
    TORCH_CHECK(u_ml.has_value(), "ce_bwd: the two-pass head needs the split (max, sum) pairs");
    CHECK_DT(*u_ml, torch::kFloat32);
    TORCH_CHECK(C == 64 && u->is_contiguous() && u->dim() == 3 && u->size(1) == M && u->size(2) == C &&
                    u_ml->is_contiguous() && u_ml->dim() == 3 && u_ml->size(0) == u->size(0) && u_ml->size(1) == M &&
                    u_ml->size(2) == 2 && u->size(0) <= 16,
                "ce_bwd: u must be (splits, M, 64) and u_ml (splits, M, 2) fp32");
    a.part_acc = u->data_ptr<float>(); a.part_ml = u_ml->data_ptr<float>(); a.nsplit = (int)u->size(0);
  }
  Tensor sl;
  if (slab) sl = torch::empty({pio::ce_bwd_slab_rows(C, M, V), (int64_t)V * C + ((V + 3) & ~3)}, dW.options());
  a.C = C; a.M = M; a.V = V;
  a.hs = bfp(h); a.labels = labels.data_ptr<int64_t>(); a.W = bfp(w); a.bias = f32p(bias);
  a.lse = f32p(lse); a.gout = f32p(gout); a.count = f32p(count);
  a.dH = dH.data_ptr<float>(); a.dh_rows = dH.size(0); a.rowmap = rm;
  a.dW = dW.data_ptr<float>(); a.db = db.data_ptr<float>(); a.accumulate = accumulate ? 1 : 0;
  a.slab = slab ? sl.data_ptr<float>() : nullptr;
  a.det = g_det ? 1 : 0;
  pio::ce_bwd_launch(a, stream());
  if (slab) return sl;
  return c10::nullopt;
}

// the k largest logits of each row of h·wᵀ + bias (row r = h[idx[r]] when idx is given, else h[r]),
// their vocabulary indices and the row's log-sum-exp over the vocabulary: → {values (M, k) fp32,
// sorted descending (the lower index first on exact ties), indices (M, k) int64, lse (M,)}.  The
// logits live in MFMA tiles only (topk_head.hip); C ∈ {64, 128}, 1 ≤ k ≤ 8, k ≤ V.
std::vector<Tensor> vocab_topk(Tensor h, OptT idx, Tensor w, Tensor bias, int64_t k) {
  CHECK_DT(h, torch::kFloat32);
  TORCH_CHECK(h.dim() == 2 && w.dim() == 2 && bias.dim() == 1, "vocab_topk: h (R, C), w (V, C), bias (V,)");
  TORCH_CHECK(h.is_contiguous() && w.is_contiguous() && bias.is_contiguous(), "vocab_topk: operands must be contiguous");
  const int C = (int)h.size(1), V = (int)w.size(0);
  TORCH_CHECK(w.size(1) == C && bias.size(0) == V && (C == 64 || C == 128), "vocab_topk: bad vocab head shape");
  TORCH_CHECK(k >= 1 && k <= 8 && k <= V, "vocab_topk: k must be in [1, min(8, V)]");
  TORCH_CHECK(w.get_device() == h.get_device() && bias.get_device() == h.get_device(), "vocab_topk: operands on one device");
  const int64_t M64 = idx.has_value() ? idx->numel() : h.size(0);
  TORCH_CHECK(M64 < (int64_t)1 << 24, "vocab_topk: too many rows");
  const int M = (int)M64;
  const int64_t* ip = nullptr;
  if (idx.has_value()) {
    CHECK_DT(*idx, torch::kInt64);
    TORCH_CHECK(idx->is_contiguous() && idx->get_device() == h.get_device(),
                "vocab_topk: idx must be a contiguous int64 tensor on the rows' device");
    ip = idx->data_ptr<int64_t>();
  }
  auto f32 = h.options().dtype(torch::kFloat32);
  Tensor values = torch::empty({M, k}, f32), indices = torch::empty({M, k}, f32.dtype(torch::kInt64));
  Tensor lse = torch::empty({M}, f32);
  if (M == 0) return {values, indices, lse};
  TORCH_CHECK(h.size(0) >= 1, "vocab_topk: no rows to gather from");
  const int ns = pio::vocab_topk_splits(M, V), kt = pio::vocab_topk_kt((int)k);
  Tensor cv = torch::empty({ns, M, kt}, f32), ci = torch::empty({ns, M, kt}, f32.dtype(torch::kInt32));
  Tensor pml = torch::empty({ns, M, 2}, f32);
  pio::VocabTopkArgs a{};
  a.C = C; a.M = M; a.V = V; a.k = (int)k;
  a.H = h.data_ptr<float>(); a.hidx = ip; a.R = h.size(0); a.W = bfp(w); a.bias = f32p(bias);
  a.nsplit = ns; a.cand_v = cv.data_ptr<float>(); a.cand_i = ci.data_ptr<int>(); a.part_ml = pml.data_ptr<float>();
  a.values = values.data_ptr<float>(); a.indices = indices.data_ptr<int64_t>(); a.lse = lse.data_ptr<float>();
  pio::vocab_topk_launch(a, stream());
  checked_sync("vocab_topk");
  return {values, indices, lse};
}

// Soft-target classifier head (soft_ce_head.hip): rows h (M, C) fp32, two labels and a weight per
// row, label smoothing eps.  → {loss (mean over the rows whose label_a is not -100), lse (M,),
// pred (M,) int32 argmax of the logits (lower class on a tie), the compact bf16 rows, count (1,)}.
// C ∈ {64, 128}, 1 ≤ V ≤ 1024.
pio::SoftCeArgs soft_ce_check(const Tensor& la, const Tensor& lb, const Tensor& lam, const Tensor& w, const Tensor& bias,
                              int M, int C, double eps) {
  CHECK_DT(la, torch::kInt64); CHECK_DT(lb, torch::kInt64); CHECK_DT(lam, torch::kFloat32);
  TORCH_CHECK(la.is_contiguous() && lb.is_contiguous() && lam.is_contiguous() && w.is_contiguous() &&
              bias.is_contiguous(), "soft_ce: operands must be contiguous");
  TORCH_CHECK(la.numel() == M && lb.numel() == M && lam.numel() == M, "soft_ce: one label pair and weight per row");
  const int64_t V = w.size(0);
  TORCH_CHECK(w.dim() == 2 && w.size(1) == C && bias.numel() == V && (C == 64 || C == 128) && V >= 1 && V <= 1024,
              "soft_ce: supported head shapes are C in {64, 128}, 1 <= V <= 1024");
  TORCH_CHECK(M >= 1 && eps >= 0.0 && eps < 1.0, "soft_ce: needs M >= 1 and eps in [0, 1)");
  for (const Tensor* t : {&la, &lb, &lam, &w, &bias}) CHECK_CUDA(*t);
  pio::SoftCeArgs a{};
  a.C = C; a.M = M; a.V = (int)V;
  a.W = bfp(w); a.bias = f32p(bias);
  a.la = la.data_ptr<int64_t>(); a.lb = lb.data_ptr<int64_t>(); a.lam = f32p(lam); a.eps = (float)eps;
  return a;
}

std::vector<Tensor> soft_ce_fwd(Tensor h, Tensor la, Tensor lb, Tensor lam, Tensor w, Tensor bias, double eps) {
  CHECK_CUDA(h);
  CHECK_DT(h, torch::kFloat32);
  TORCH_CHECK(h.dim() == 2 && h.is_contiguous() && h.size(0) < (1 << 24), "soft_ce_fwd: h must be (M, C) contiguous");
  const int M = (int)h.size(0), C = (int)h.size(1);
  pio::SoftCeArgs a = soft_ce_check(la, lb, lam, w, bias, M, C, eps);
  auto f32 = h.options().dtype(torch::kFloat32);
  const int nrt = pio::soft_ce_row_tiles(M);
  Tensor loss = torch::empty({}, f32), lse = torch::empty({M}, f32), count = torch::empty({1}, f32);
  Tensor pred = torch::empty({M}, f32.dtype(torch::kInt32)), hs = torch::empty({M, C}, f32.dtype(torch::kBFloat16));
  Tensor blk = torch::empty({2 * nrt}, f32);
  a.H = h.data_ptr<float>(); a.hs = bfp_mut(hs); a.lse = lse.data_ptr<float>(); a.count = count.data_ptr<float>();
  a.pred = pred.data_ptr<int>(); a.blk = blk.data_ptr<float>(); a.loss = loss.data_ptr<float>();
  pio::soft_ce_fwd_launch(a, stream());
  checked_sync("soft_ce_fwd");
  return {loss, lse, pred, hs, count};
}

// hs: the compact bf16 rows of soft_ce_fwd.  dH (M, C) is overwritten; dW / db are added to
// (accumulate) or overwritten.
void soft_ce_bwd(Tensor hs, Tensor la, Tensor lb, Tensor lam, Tensor w, Tensor bias, double eps, Tensor lse, Tensor gout,
                 Tensor count, Tensor dH, Tensor dW, Tensor db, bool accumulate) {
  CHECK_CUDA(hs);
  TORCH_CHECK(hs.dim() == 2 && hs.is_contiguous(), "soft_ce_bwd: hs must be the compact (M, C) bf16 rows");
  const int M = (int)hs.size(0), C = (int)hs.size(1), V = (int)w.size(0);
  pio::SoftCeArgs a = soft_ce_check(la, lb, lam, w, bias, M, C, eps);
  for (const Tensor* t : {&lse, &gout, &count, &dH, &dW, &db}) {
    CHECK_CUDA(*t); CHECK_DT(*t, torch::kFloat32);
    TORCH_CHECK(t->is_contiguous(), "soft_ce_bwd: operands must be contiguous");
  }
  TORCH_CHECK(lse.numel() == M && gout.numel() >= 1 && count.numel() >= 1, "soft_ce_bwd: bad lse / gout / count");
  TORCH_CHECK(dH.numel() == (int64_t)M * C && dW.numel() == (int64_t)V * C && db.numel() == V,
              "soft_ce_bwd: dH (M, C), dW (V, C), db (V,)");
  a.hs = bfp_mut(hs); a.lse = lse.data_ptr<float>(); a.count = count.data_ptr<float>();  // read only here
  a.gout = f32p(gout); a.dH = dH.data_ptr<float>(); a.dW = dW.data_ptr<float>(); a.db = db.data_ptr<float>();
  a.accumulate = accumulate ? 1 : 0;
  pio::soft_ce_bwd_launch(a, stream());
}

// MixUp / CutMix of a channels-last batch with its flipped self; mix = {mode, lambda, y0, y1, x0, x1}
// as fp32 words on the device (read by the kernel).  → {mixed x, label_b, lam (B,)}
std::vector<Tensor> batch_mix(Tensor x, Tensor y, Tensor mix) {
  CHECK_CUDA(x); CHECK_CUDA(y); CHECK_CUDA(mix);
  CHECK_DT(x, torch::kFloat32); CHECK_DT(y, torch::kInt64); CHECK_DT(mix, torch::kFloat32);
  TORCH_CHECK(x.dim() == 4 && x.is_contiguous() && y.is_contiguous() && mix.is_contiguous(),
              "batch_mix: x must be (B, H, W, Ch) contiguous");
  TORCH_CHECK(y.numel() == x.size(0) && mix.numel() >= 6 && x.size(0) >= 1, "batch_mix: y (B,), mix (6,)");
  const int64_t n = x.size(1) * x.size(2) * x.size(3);
  TORCH_CHECK(n >= 1 && n < ((int64_t)1 << 30) && x.size(0) < (1 << 16), "batch_mix: sample too large");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0, "batch_mix: x must be 16-byte aligned");
  Tensor out = torch::empty_like(x), yb = torch::empty_like(y);
  Tensor lam = torch::empty({x.size(0)}, x.options());
  pio::batch_mix_launch(x.data_ptr<float>(), y.data_ptr<int64_t>(), f32p(mix), out.data_ptr<float>(),
                        yb.data_ptr<int64_t>(), lam.data_ptr<float>(), (int)x.size(0), (int)x.size(1), (int)x.size(2),
                        (int)x.size(3), stream());
  return {out, yb, lam};
}

// crop box → bilinear resize → horizontal flip → normalize of a raw uint8 channels-last batch (csrc/augment.hip);
// params (B, 8) fp32 on the device: {y0, x0, h, w, flip, 0, 0, 0} per sample, read by the kernel
Tensor batch_augment(Tensor src, Tensor params, std::vector<double> mean, std::vector<double> std_, int64_t out_h,
                     int64_t out_w) {
  CHECK_CUDA(src); CHECK_CUDA(params);
  CHECK_DT(src, torch::kUInt8); CHECK_DT(params, torch::kFloat32);
  TORCH_CHECK(src.dim() == 4 && src.is_contiguous(), "batch_augment: src must be (B, Hs, Ws, C) uint8 contiguous");
  const int64_t B = src.size(0), Hs = src.size(1), Ws = src.size(2), C = src.size(3);
  TORCH_CHECK(B >= 1 && B < (1 << 16) && Hs >= 1 && Ws >= 1, "batch_augment: 1 <= B < 65536, a non-empty source");
  TORCH_CHECK(C >= 1 && C <= 4, "batch_augment: 1 to 4 channels, got ", C);
  TORCH_CHECK((int64_t)mean.size() == C && (int64_t)std_.size() == C, "batch_augment: mean / std need one value per channel");
  TORCH_CHECK(params.dim() == 2 && params.size(0) == B && params.size(1) == 8 && params.is_contiguous() &&
                  params.get_device() == src.get_device(),
              "batch_augment: params must be (B, 8) fp32 contiguous on src's device");
  TORCH_CHECK(out_h >= 1 && out_w >= 1, "batch_augment: out_hw must be positive");
  const int64_t lim = (int64_t)1 << 30;
  TORCH_CHECK(Hs * Ws * C < lim && out_h * out_w * C < lim && Hs < lim && Ws < lim && out_h < lim && out_w < lim,
              "batch_augment: a sample (source or output) must hold fewer than 2^30 elements");
  float mv[4], sv[4];
  for (int64_t c = 0; c < C; ++c) {
    mv[c] = (float)mean[c];
    sv[c] = (float)std_[c];
  }
  Tensor out = torch::empty({B, out_h, out_w, C}, src.options().dtype(torch::kFloat32));
  pio::batch_augment_launch(src.data_ptr<uint8_t>(), f32p(params), out.data_ptr<float>(), (int)B, (int)Hs, (int)Ws, (int)C,
                            (int)out_h, (int)out_w, mv, sv, stream());
  // no checked_sync: a clamped box has a defined result; the checked build's bit 16 waits for check_errors
  return out;
}

// RandAugment of a raw uint8 channels-last batch (csrc/randaugment.hip): words (B, N, 8) fp32 on the device,
// {op, v, m00, m01, m02, m10, m11, m12} per sample and layer, read by the kernels.  The ping-pong image and the
// histogram block come from the current allocator: inside a capture, from the graph's private pool.
Tensor rand_augment(Tensor src, Tensor words, int64_t fill) {
  CHECK_CUDA(src); CHECK_CUDA(words);
  CHECK_DT(src, torch::kUInt8); CHECK_DT(words, torch::kFloat32);
  TORCH_CHECK(src.dim() == 4 && src.is_contiguous(), "rand_augment: src must be (B, H, W, C) uint8 contiguous");
  const int64_t B = src.size(0), H = src.size(1), W = src.size(2), C = src.size(3);
  TORCH_CHECK(B >= 1 && B < (1 << 16) && H >= 1 && W >= 1, "rand_augment: 1 <= B < 65536, a non-empty image");
  TORCH_CHECK(C == 1 || C == 3, "rand_augment: 1 or 3 channels, got ", C);
  const int64_t lim = (int64_t)1 << 30;
  TORCH_CHECK(H < lim && W < lim && H * W * C < lim, "rand_augment: a sample must hold fewer than 2^30 elements");
  TORCH_CHECK(words.dim() == 3 && words.size(0) == B && words.size(2) == 8 && words.is_contiguous() &&
                  words.get_device() == src.get_device(),
              "rand_augment: words must be (B, N, 8) fp32 contiguous on src's device");
  const int64_t N = words.size(1);
  TORCH_CHECK(N >= 1 && N <= 8, "rand_augment: 1 <= N <= 8 layers, got ", N);
  TORCH_CHECK(fill >= 0 && fill <= 255, "rand_augment: fill must be a uint8 value");
  Tensor out = torch::empty_like(src);
  Tensor tmp = N > 1 ? torch::empty_like(src) : Tensor();
  // a fill kernel on the stream (not a memset, which a captured graph would not replay): zero on every replay
  Tensor hist = torch::zeros({N, B, C + 1, 256}, src.options().dtype(torch::kInt32));
  pio::rand_augment_launch(src.data_ptr<uint8_t>(), f32p(words), out.data_ptr<uint8_t>(),
                           N > 1 ? tmp.data_ptr<uint8_t>() : nullptr, hist.data_ptr<int>(), (int)B, (int)H, (int)W, (int)C,
                           (int)N, (int)fill, stream());
  // no checked_sync: an op word outside the table is identity; the checked build's bit 32 waits for check_errors
  return out;
}

Tensor embed_fwd(Tensor ids, Tensor E, Tensor P, double scale) {
  TORCH_CHECK(ids.is_contiguous() && E.is_contiguous() && P.is_contiguous());
  CHECK_DT(ids, torch::kInt64);
  const long long rows = ids.numel();
  const int L = (int)ids.size(1), C = (int)E.size(1);
  TORCH_CHECK(C % 4 == 0, "embedding width must be a multiple of 4");
  Tensor out = torch::empty({ids.size(0), L, C}, E.options());
  pio::embed_fwd_launch(ids.data_ptr<int64_t>(), f32p(E), f32p(P), out.data_ptr<float>(), rows, L, C, (float)scale,
                        E.size(0), stream());
  checked_sync("embed_fwd");
  return out;
}

// The text encoder's input pass: the embedding and both cross layers' LayerNorm + K|V projection
// in one launch.  la / lb = [lnw (64), lnb (64), w bf16 (128, 64), bias (128)] of layer_1 /
// layer_n; returns (x (B, L, 64) fp32, mean, rstd, kv_a, kv_b (B·L, 128) bf16).
std::vector<Tensor> text_kv_fwd(Tensor ids, Tensor E, Tensor P, double scale, double eps, std::vector<Tensor> la,
                                std::vector<Tensor> lb) {
  CHECK_CUDA(ids); CHECK_CUDA(E);
  TORCH_CHECK(ids.dim() == 2 && ids.is_contiguous() && E.is_contiguous() && P.is_contiguous());
  CHECK_DT(ids, torch::kInt64);
  const int64_t B = ids.size(0), L = ids.size(1), R = B * L;
  TORCH_CHECK(E.dim() == 2 && E.size(1) == 64 && P.dim() == 2 && P.size(1) == 64 && P.size(0) >= L,
              "text_kv_fwd: 64-channel embedding and position tables, at least L positions");
  TORCH_CHECK(R > 0 && R < (int64_t(1) << 31), "text_kv_fwd: bad row count");
  TORCH_CHECK(la.size() == 4 && lb.size() == 4, "text_kv_fwd: [lnw, lnb, w, bias] per layer");
  auto opts = E.options();
  Tensor x = torch::empty({B, L, 64}, opts);
  Tensor mean = torch::empty({R}, opts), rstd = torch::empty({R}, opts);
  Tensor kva = torch::empty({R, 128}, opts.dtype(torch::kBFloat16)), kvb = torch::empty({R, 128}, opts.dtype(torch::kBFloat16));
  auto proj = [](std::vector<Tensor>& l, Tensor& kv) {
    TORCH_CHECK(l[0].is_contiguous() && l[0].numel() == 64 && l[1].is_contiguous() && l[1].numel() == 64,
                "text_kv_fwd: LN affine of 64 channels");
    TORCH_CHECK(l[2].dim() == 2 && l[2].is_contiguous() && l[2].size(0) == 128 && l[2].size(1) == 64,
                "text_kv_fwd: w must be (128, 64) contiguous");
    TORCH_CHECK(l[3].is_contiguous() && l[3].numel() == 128, "text_kv_fwd: bias of 128 columns");
    return pio::TextKvProj{f32p(l[0]), f32p(l[1]), bfp(l[2]), f32p(l[3]), bfp_mut(kv)};
  };
  pio::TextKvFwdArgs a{};
  a.ids = ids.data_ptr<int64_t>();
  a.E = f32p(E);
  a.P = f32p(P);
  a.scale = (float)scale;
  a.V = E.size(0);
  a.L = (int)L;
  a.R = (int)R;
  a.eps = (float)eps;
  a.a = proj(la, kva);
  a.b = proj(lb, kvb);
  a.X = x.data_ptr<float>();
  a.mean = mean.data_ptr<float>();
  a.rstd = rstd.data_ptr<float>();
  TORCH_CHECK(pio::text_kv_fwd_launch(a, stream()), "text_kv_fwd: operands must be 16-byte aligned");
  checked_sync("text_kv_fwd");
  return {x, mean, rstd, kva, kvb};
}

// dx (R, 64) = LN_bwd over both layers' dK|dV (ga / gb fp32 (R, 128)); la / lb = [lnw, lnb, w bf16];
// grads = [dlnw, dlnb, dW, db] of layer a then of layer b: plain / replicated accumulators, or
// (slab) (ceil(R / 64), ·) views of ONE slab (see vec_target)
Tensor text_kv_bwd(Tensor ga, Tensor gb, Tensor x, Tensor mean, Tensor rstd, std::vector<Tensor> la,
                   std::vector<Tensor> lb, std::vector<Tensor> grads, bool slab, OptT job_slab,
                   std::vector<Tensor> job_dsts, std::vector<int64_t> job_offs) {
  CHECK_CUDA(ga); CHECK_CUDA(x);
  const int64_t R = ga.size(0);
  TORCH_CHECK(ga.dim() == 2 && ga.is_contiguous() && ga.size(1) == 128 && gb.is_contiguous() && gb.dim() == 2 &&
                  gb.size(0) == R && gb.size(1) == 128,
              "text_kv_bwd: dK|dV must be (R, 128) contiguous");
  TORCH_CHECK(x.is_contiguous() && x.numel() == R * 64 && mean.is_contiguous() && mean.numel() == R &&
                  rstd.is_contiguous() && rstd.numel() == R,
              "text_kv_bwd: x (R, 64) and its row statistics");
  TORCH_CHECK(R > 0 && R < kTallRows, "text_kv_bwd: bad row count");
  TORCH_CHECK(!g_det || slab, "deterministic mode: text_kv_bwd parameter gradients need slab mode");
  TORCH_CHECK(la.size() == 3 && lb.size() == 3 && grads.size() == 8, "text_kv_bwd: [lnw, lnb, w] per layer, 8 targets");
  const int64_t sr = slab ? (R + 63) / 64 : 0;
  int vrs = -1;
  auto layer = [&](const Tensor& g, std::vector<Tensor>& l, int t0) {
    TORCH_CHECK(l[0].is_contiguous() && l[0].numel() == 64 && l[1].is_contiguous() && l[1].numel() == 64,
                "text_kv_bwd: LN affine of 64 channels");
    TORCH_CHECK(l[2].dim() == 2 && l[2].is_contiguous() && l[2].size(0) == 128 && l[2].size(1) == 64,
                "text_kv_bwd: w must be (128, 64) contiguous");
    pio::TextKvGrad o{};
    o.G = f32p(g);
    o.lnw = f32p(l[0]);
    o.lnb = f32p(l[1]);
    o.W = bfp(l[2]);
    o.dlnw = vec_target(grads[t0], 64, "dlnw", vrs, sr);
    o.dlnb = vec_target(grads[t0 + 1], 64, "dlnb", vrs, sr);
    o.dW = vec_target(grads[t0 + 2], 128 * 64, "dW", vrs, sr);
    o.db = vec_target(grads[t0 + 3], 128, "db", vrs, sr);
    return o;
  };
  Tensor dx = torch::empty({R, 64}, ga.options());
  pio::TextKvBwdArgs a{};
  a.a = layer(ga, la, 0);
  a.b = layer(gb, lb, 4);
  a.X = f32p(x);
  a.mean = f32p(mean);
  a.rstd = f32p(rstd);
  a.dX = dx.data_ptr<float>();
  a.vrs = vrs < 0 ? 0 : vrs;
  a.slab = slab ? 1 : 0;
  a.R = (int)R;
  a.job = make_job(job_slab, job_dsts, job_offs);
  TORCH_CHECK(pio::text_kv_bwd_launch(a, stream()), "text_kv_bwd: operands must be 16-byte aligned");
  return dx;
}

void embed_bwd(Tensor ids, Tensor g, OptT dE, OptT dP, double scale, OptT job_slab, std::vector<Tensor> job_dsts,
               std::vector<int64_t> job_offs) {
  TORCH_CHECK(g.is_contiguous() && ids.is_contiguous());
  const pio::SlabJob job = make_job(job_slab, job_dsts, job_offs);
  const int B = (int)ids.size(0), L = (int)ids.size(1), C = (int)g.size(2);
  if (dE.has_value()) TORCH_CHECK(dE->is_contiguous() && dE->size(1) == C, "dE must be (V, C) contiguous");
  if (dP.has_value()) TORCH_CHECK(dP->is_contiguous() && dP->size(1) == C && dP->size(0) >= L, "dP must be (>= L, C)");
  // one launch: block-local sort + run folding for dE, batch sums for dP (C ∈ {64, 128, 256}, ids < 2^24)
  if ((!dE.has_value() || dE->size(0) < (1 << 24)) &&
      pio::embed_bwd_local_launch(ids.data_ptr<int64_t>(), f32p(g), dE.has_value() ? dE->data_ptr<float>() : nullptr,
                                  dP.has_value() ? dP->data_ptr<float>() : nullptr, B, L, C, (float)scale, job,
                                  stream()))
    return;
  if (job.slab) pio::slab_reduce_launch(job, stream());  // the fallback paths carry no job
  if (dE.has_value()) {  // token-embedding rows: sort positions by id, fold equal-id runs, then add
    TORCH_CHECK(dE->is_contiguous() && dE->size(1) == C, "dE must be (V, C) contiguous");
    const bool small = dE->size(0) <= 32767;  // int16 keys: a 2-pass radix sort instead of 8
    Tensor keys = small ? ids.reshape({-1}).to(torch::kInt16) : ids.reshape({-1});
    auto sorted = keys.sort();
    Tensor sid = std::get<0>(sorted).to(torch::kInt64).contiguous(), perm = std::get<1>(sorted).contiguous();
    pio::embed_bwd_sorted_launch(sid.data_ptr<int64_t>(), perm.data_ptr<int64_t>(), f32p(g), dE->data_ptr<float>(),
                                 ids.numel(), C, (float)scale, stream());
  }
  if (dP.has_value())
    pio::embed_bwd_launch(ids.data_ptr<int64_t>(), f32p(g), nullptr, dP->data_ptr<float>(), B, L, C, (float)scale,
                          stream());
}

// state: int64 (3,) {seed, counter, ticket} on the device (see text_mask_kernel); advance: the
// launch increments the counter (fresh masks on every call / graph replay)
std::vector<Tensor> text_mask(Tensor x, OptT pad, Tensor state, int64_t unk, int64_t mask, double p, int64_t lo,
                              int64_t hi, bool advance) {
  TORCH_CHECK(x.is_contiguous() && state.is_contiguous() && state.numel() == 3, "text_mask: bad x / state");
  CHECK_DT(x, torch::kInt64);
  CHECK_DT(state, torch::kInt64);
  TORCH_CHECK(hi > lo && hi - lo < (1LL << 32), "text_mask: bad random-id range");
  const long long n = x.numel();
  TORCH_CHECK(n < (1LL << 32), "text_mask: too many tokens");
  Tensor xm = torch::empty_like(x), lab = torch::empty_like(x);
  const bool* pp = nullptr;
  if (pad.has_value()) {
    CHECK_DT(*pad, torch::kBool);
    TORCH_CHECK(pad->is_contiguous() && pad->numel() == n, "text_mask: pad mask must match x");
    pp = pad->data_ptr<bool>();
  }
  pio::text_mask_launch(x.data_ptr<int64_t>(), pp, state.data_ptr<int64_t>(), xm.data_ptr<int64_t>(),
                        lab.data_ptr<int64_t>(), n, (int)unk, (int)mask, (float)p, (int)lo, (uint32_t)(hi - lo),
                        advance ? 1 : 0, stream());
  return {xm, lab};
}

// whole-word masking (text_mask_words_kernel): x (B, L); table: the vocabulary's bit-packed
// continuation table, int32 (⌈hi / 32⌉,) on x's device — hi is the vocabulary size
std::vector<Tensor> text_mask_words(Tensor x, OptT pad, Tensor state, Tensor table, int64_t unk, int64_t mask, double p,
                                    int64_t lo, int64_t hi, bool advance) {
  TORCH_CHECK(x.is_contiguous() && state.is_contiguous() && state.numel() == 3, "text_mask_words: bad x / state");
  TORCH_CHECK(x.dim() == 2 && x.size(1) > 0, "text_mask_words: x must be (B, L)");
  CHECK_CUDA(x);
  CHECK_DT(x, torch::kInt64);
  CHECK_DT(state, torch::kInt64);
  CHECK_DT(table, torch::kInt32);
  TORCH_CHECK(hi > lo && hi - lo < (1LL << 32), "text_mask_words: bad random-id range");
  TORCH_CHECK(hi < (1LL << 31), "text_mask_words: vocabulary too large");
  TORCH_CHECK(table.is_contiguous() && table.dim() == 1 && table.numel() == (hi + 31) / 32,
              "text_mask_words: the continuation table must hold ceil(hi / 32) packed words");
  TORCH_CHECK(table.device() == x.device() && state.device() == x.device(),
              "text_mask_words: table and state must be on x's device");
  const long long n = x.numel();
  TORCH_CHECK(n < (1LL << 32), "text_mask_words: too many tokens");
  TORCH_CHECK(x.size(1) < (1LL << 31), "text_mask_words: rows too long");
  Tensor xm = torch::empty_like(x), lab = torch::empty_like(x);
  const bool* pp = nullptr;
  if (pad.has_value()) {
    CHECK_DT(*pad, torch::kBool);
    TORCH_CHECK(pad->is_contiguous() && pad->numel() == n && pad->device() == x.device(),
                "text_mask_words: pad mask must match x");
    pp = pad->data_ptr<bool>();
  }
  pio::text_mask_words_launch(x.data_ptr<int64_t>(), pp, state.data_ptr<int64_t>(), table.data_ptr<int32_t>(),
                              xm.data_ptr<int64_t>(), lab.data_ptr<int64_t>(), n, (int)x.size(1), (int)hi, (int)unk,
                              (int)mask, (float)p, (int)lo, (uint32_t)(hi - lo), advance ? 1 : 0, stream());
  return {xm, lab};
}

// one launch per replayed step: dsts[i] <- srcs[i] (same device, dtype-agnostic byte copies of
// contiguous tensors of equal size) and hyper_dst[:len(hyper)] <- hyper (values by kernel argument)
// seed_dst + seeds: a captured step's dropout seed slots (int64, ≤ 64 values) written in the same launch
void stage_step(std::vector<Tensor> dsts, std::vector<Tensor> srcs, OptT hyper_dst, std::vector<double> hyper,
                OptT seed_dst, std::vector<int64_t> seeds) {
  TORCH_CHECK(dsts.size() == srcs.size() && dsts.size() <= 8 && hyper.size() <= 40, "stage_step: at most 8 tensors / 40 values");
  std::vector<void*> d;
  std::vector<const void*> x;
  std::vector<long long> n;
  for (size_t i = 0; i < dsts.size(); ++i) {
    const Tensor& a = dsts[i];
    const Tensor& b = srcs[i];
    TORCH_CHECK(a.is_cuda() && b.is_cuda() && a.get_device() == b.get_device() && a.is_contiguous() && b.is_contiguous() &&
                    a.scalar_type() == b.scalar_type() && a.numel() == b.numel(),
                "stage_step: pairs must be contiguous same-device tensors of equal dtype and size");
    d.push_back(a.data_ptr());
    x.push_back(b.data_ptr());
    n.push_back((long long)(a.numel() * a.element_size()));
  }
  float* hp = nullptr;
  std::vector<float> hv(hyper.begin(), hyper.end());
  if (hyper_dst.has_value()) {
    CHECK_DT(*hyper_dst, torch::kFloat32);
    TORCH_CHECK(hyper_dst->is_contiguous() && hyper_dst->numel() >= (int64_t)hv.size(), "stage_step: hyper_dst too small");
    hp = hyper_dst->data_ptr<float>();
  }
  long long* sp = nullptr;
  if (!seeds.empty()) {
    TORCH_CHECK(seed_dst.has_value() && seed_dst->is_cuda() && seed_dst->is_contiguous() &&
                    seed_dst->scalar_type() == torch::kInt64 && seed_dst->numel() >= (int64_t)seeds.size() &&
                    seeds.size() <= 64,
                "stage_step: seed_dst must be a contiguous int64 device tensor of >= len(seeds) (<= 64) slots");
    sp = reinterpret_cast<long long*>(seed_dst->data_ptr<int64_t>());
  }
  std::vector<long long> sv(seeds.begin(), seeds.end());
  TORCH_CHECK(pio::stage_step_launch(d.data(), x.data(), n.data(), (int)d.size(), hp, hv.data(), (int)hv.size(), sp,
                                     sv.data(), (int)sv.size(), stream()) == 0);
}

// Σ g² as kSumsqBlocks fixed-order partials (part: ≥ kSumsqBlocks fp32), read by adamw(norm_part=)
constexpr int kSumsqParts = 512;  // common.h kSumsqBlocks
void sumsq(Tensor g, Tensor part) {
  CHECK_DT(g, torch::kFloat32); CHECK_DT(part, torch::kFloat32);
  TORCH_CHECK(g.is_contiguous() && part.is_contiguous() && part.numel() >= kSumsqParts,
              "sumsq: contiguous gradient, a contiguous partial buffer of >= 512 floats");
  pio::sumsq_launch(f32p(g), g.numel(), part.data_ptr<float>(), stream());
}

// a, b: (B, ...) fp32 contiguous, equal shapes → (Σ_b a[b], Σ_b b[b]) in one launch
// oa = Σ_b a[b] (a optional), ob = Σ_b b[b] — or, with ob_acc, ob_acc += Σ_b b[b] in place (the
// gradient of a batch-broadcast parameter straight into its gradient buffer)
std::vector<Tensor> batch_sum2(OptT a, Tensor b, OptT ob_acc) {
  CHECK_DT(b, torch::kFloat32);
  TORCH_CHECK(b.is_contiguous() && b.dim() >= 2, "batch_sum2: b must be contiguous (B, ...)");
  const long long n = b.numel() / b.size(0);
  TORCH_CHECK(n % 4 == 0 && reinterpret_cast<uintptr_t>(b.data_ptr()) % 16 == 0, "batch_sum2: 16-byte rows");
  if (a.has_value()) {
    CHECK_DT(*a, torch::kFloat32);
    TORCH_CHECK(a->is_contiguous() && a->sizes() == b.sizes() && reinterpret_cast<uintptr_t>(a->data_ptr()) % 16 == 0,
                "batch_sum2: a must match b");
  }
  std::vector<int64_t> shp(b.sizes().begin() + 1, b.sizes().end());
  Tensor oa = a.has_value() ? torch::empty(shp, b.options()) : Tensor();
  Tensor ob;
  if (ob_acc.has_value()) {
    CHECK_DT(*ob_acc, torch::kFloat32);
    TORCH_CHECK(ob_acc->is_contiguous() && ob_acc->numel() == n && reinterpret_cast<uintptr_t>(ob_acc->data_ptr()) % 16 == 0,
                "batch_sum2: ob_acc must be a contiguous, 16-byte aligned tensor of one batch element's size");
    ob = ob_acc->view(shp);
  } else {
    ob = torch::empty(shp, b.options());
  }
  pio::batch_sum2_launch(a.has_value() ? a->data_ptr<float>() : nullptr, b.data_ptr<float>(),
                         a.has_value() ? oa.data_ptr<float>() : nullptr, ob.data_ptr<float>(), (int)b.size(0), n, n,
                         ob_acc.has_value() ? 1 : 0, stream());
  return {oa, ob};
}

// dst (N, C) fp32 += src (R, C) fp32 scattered to rows idx (R) — the backward of a row gather
void index_add_rows(Tensor dst, Tensor idx, Tensor src) {
  CHECK_DT(dst, torch::kFloat32); CHECK_DT(src, torch::kFloat32); CHECK_DT(idx, torch::kInt64);
  TORCH_CHECK(dst.dim() == 2 && dst.is_contiguous() && src.dim() == 2 && src.is_contiguous() && idx.is_contiguous(),
              "index_add_rows: contiguous dst (N, C), src (R, C), idx (R)");
  TORCH_CHECK(src.size(1) == dst.size(1) && idx.numel() == src.size(0) && dst.size(1) % 4 == 0,
              "index_add_rows: shapes (C % 4 == 0)");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(dst.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(src.data_ptr()) % 16 == 0,
              "index_add_rows: 16-byte aligned rows");
  if (src.size(0) == 0) return;
  pio::index_add_rows_launch(dst.data_ptr<float>(), dst.size(0), idx.data_ptr<int64_t>(), f32p(src), src.size(0),
                             (int)src.size(1), stream());
  checked_sync("index_add_rows");
}

// src (N, C) fp32 rows at idx (R) → (R, C) — a row gather (decoder output queries of a sparse image)
Tensor gather_rows(Tensor src, Tensor idx) {
  CHECK_DT(src, torch::kFloat32); CHECK_DT(idx, torch::kInt64);
  TORCH_CHECK(src.dim() == 2 && src.is_contiguous() && idx.is_contiguous() && src.size(1) % 4 == 0 &&
                  reinterpret_cast<uintptr_t>(src.data_ptr()) % 16 == 0,
              "gather_rows: contiguous 16-byte aligned src (N, C), C % 4 == 0, contiguous idx");
  Tensor out = torch::empty({idx.numel(), src.size(1)}, src.options());
  if (idx.numel() == 0) return out;
  pio::gather_rows_launch(out.data_ptr<float>(), f32p(src), src.size(0), idx.data_ptr<int64_t>(), idx.numel(),
                          (int)src.size(1), stream());
  checked_sync("gather_rows");
  return out;
}

namespace {
void check_pixel_head(const Tensor& h, const Tensor& w, const Tensor& b, const Tensor& labels, const Tensor& wts) {
  CHECK_DT(h, torch::kFloat32); CHECK_DT(w, torch::kFloat32); CHECK_DT(b, torch::kFloat32);
  CHECK_DT(labels, torch::kInt64); CHECK_DT(wts, torch::kFloat32);
  TORCH_CHECK(h.dim() == 2 && h.is_contiguous() && w.dim() == 2 && w.is_contiguous() && b.is_contiguous() &&
                  labels.is_contiguous() && wts.is_contiguous(), "pixel head: contiguous h (R, C), w (K, C)");
  const int C = (int)h.size(1), K = (int)w.size(0);
  TORCH_CHECK((C == 32 || C == 64 || C == 128) && K >= 2 && K <= 4 && w.size(1) == C && b.numel() == K &&
                  wts.numel() == K && labels.numel() == h.size(0), "pixel head: C in {32, 64, 128}, 2 <= K <= 4");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(h.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 == 0,
              "pixel head: 16-byte aligned rows");
}
}  // namespace

// → [stats (4 + 2K sums: Σ w·ce, Σ w, n(lab>0), hit(lab>0), (n_k, hit_k)… | acc, acc_1 … acc_{K-1}),
//    loss = Σ w·ce / Σ w (0-dim)]
std::vector<Tensor> pixel_ce_fwd(Tensor h, Tensor w, Tensor b, Tensor labels, Tensor wts) {
  check_pixel_head(h, w, b, labels, wts);
  const long long R = h.size(0);
  const int K = (int)w.size(0);
  // every block of the launch stores its whole partial row (zeros only for an empty input)
  Tensor part = R > 0 ? torch::empty({pio::pixel_ce_blocks(R), 4 + 2 * K}, h.options())
                      : torch::zeros({pio::pixel_ce_blocks(R), 4 + 2 * K}, h.options());
  Tensor stats = torch::empty({4 + 2 * K + K}, h.options()), loss = torch::empty({}, h.options());
  pio::pixel_ce_fwd_launch((int)h.size(1), K, f32p(h), f32p(w), f32p(b), labels.data_ptr<int64_t>(), f32p(wts), R,
                           part.data_ptr<float>(), stats.data_ptr<float>(), loss.data_ptr<float>(), stream());
  return {stats, loss};
}

// dH (R, C) written; dW (K, C) / db (K) += the head's weight gradients (fixed-order sums)
void pixel_ce_bwd(Tensor h, Tensor w, Tensor b, Tensor labels, Tensor wts, Tensor gout, Tensor stats, Tensor dH,
                  Tensor dW, Tensor db) {
  check_pixel_head(h, w, b, labels, wts);
  CHECK_DT(gout, torch::kFloat32); CHECK_DT(stats, torch::kFloat32); CHECK_DT(dH, torch::kFloat32);
  CHECK_DT(dW, torch::kFloat32); CHECK_DT(db, torch::kFloat32);
  TORCH_CHECK(dH.is_contiguous() && dH.sizes() == h.sizes() && gout.numel() == 1 && stats.numel() >= 2,
              "pixel head bwd: dH like h, scalar loss gradient");
  TORCH_CHECK(dW.is_contiguous() && dW.numel() == w.numel() && db.is_contiguous() && db.numel() == b.numel(),
              "pixel head bwd: dW / db like w / b");
  const long long R = h.size(0);
  const int K = (int)w.size(0), C = (int)h.size(1);
  Tensor part = R > 0 ? torch::empty({pio::pixel_ce_blocks(R), (int64_t)K * C + K}, h.options())
                      : torch::zeros({pio::pixel_ce_blocks(R), (int64_t)K * C + K}, h.options());
  pio::pixel_ce_bwd_launch(C, K, f32p(h), f32p(w), f32p(b), labels.data_ptr<int64_t>(), f32p(wts), f32p(gout),
                           f32p(stats), R, dH.data_ptr<float>(), part.data_ptr<float>(), dW.data_ptr<float>(),
                           db.data_ptr<float>(), stream());
}

namespace {
void check_seg_loss(const Tensor& h, const Tensor& w, const Tensor& b, const Tensor& labels, const Tensor& wts,
                    double gamma, double ce_weight, double dice_weight, double eps) {
  check_pixel_head(h, w, b, labels, wts);
  CHECK_CUDA(h);
  TORCH_CHECK(w.get_device() == h.get_device() && b.get_device() == h.get_device() &&
                  labels.get_device() == h.get_device() && wts.get_device() == h.get_device(),
              "pixel seg: every operand on h's device");
  // written so that a NaN fails each rule
  TORCH_CHECK(gamma >= 0.0 && std::isfinite(gamma), "pixel seg: focal gamma must be >= 0, got ", gamma);
  TORCH_CHECK(ce_weight >= 0.0 && dice_weight >= 0.0 && std::isfinite(ce_weight) && std::isfinite(dice_weight) &&
                  ce_weight + dice_weight > 0.0,
              "pixel seg: ce_weight and dice_weight must be >= 0 and not both 0, got ", ce_weight, ", ", dice_weight);
  TORCH_CHECK(eps > 0.0 && std::isfinite(eps), "pixel seg: dice eps must be > 0, got ", eps);
}
}  // namespace

// Focal cross-entropy + soft Dice of the head (pixel_head.hip pixel_seg_*; the definition is there) →
// [stats (4 + 5K sums: the 4 + 2K of pixel_ce_fwd with Σ w·q^γ·ce first, then I_c, P_c, T_c | acc,
//  acc_1 … acc_{K-1} | F, D | the K per-class soft Dice coefficients), loss (0-dim)]
std::vector<Tensor> pixel_seg_fwd(Tensor h, Tensor w, Tensor b, Tensor labels, Tensor wts, double gamma,
                                  double ce_weight, double dice_weight, double eps) {
  check_seg_loss(h, w, b, labels, wts, gamma, ce_weight, dice_weight, eps);
  const long long R = h.size(0);
  const int K = (int)w.size(0);
  // every block of the launch stores its whole partial row (zeros only for an empty input)
  Tensor part = R > 0 ? torch::empty({pio::pixel_ce_blocks(R), 4 + 5 * K}, h.options())
                      : torch::zeros({pio::pixel_ce_blocks(R), 4 + 5 * K}, h.options());
  Tensor stats = torch::empty({6 + 7 * K}, h.options()), loss = torch::empty({}, h.options());
  pio::pixel_seg_fwd_launch((int)h.size(1), K, f32p(h), f32p(w), f32p(b), labels.data_ptr<int64_t>(), f32p(wts),
                            (float)gamma, (float)ce_weight, (float)dice_weight, (float)eps, R, part.data_ptr<float>(),
                            stats.data_ptr<float>(), loss.data_ptr<float>(), stream());
  return {stats, loss};
}

// dH (R, C) written; dW (K, C) / db (K) += the head's weight gradients (fixed-order sums); stats is
// pixel_seg_fwd's, computed with the same parameters
void pixel_seg_bwd(Tensor h, Tensor w, Tensor b, Tensor labels, Tensor wts, double gamma, double ce_weight,
                   double dice_weight, double eps, Tensor gout, Tensor stats, Tensor dH, Tensor dW, Tensor db) {
  check_seg_loss(h, w, b, labels, wts, gamma, ce_weight, dice_weight, eps);
  CHECK_DT(gout, torch::kFloat32); CHECK_DT(stats, torch::kFloat32); CHECK_DT(dH, torch::kFloat32);
  CHECK_DT(dW, torch::kFloat32); CHECK_DT(db, torch::kFloat32);
  const long long R = h.size(0);
  const int K = (int)w.size(0), C = (int)h.size(1);
  TORCH_CHECK(dH.is_contiguous() && dH.sizes() == h.sizes() && gout.numel() == 1 && stats.is_contiguous() &&
                  stats.numel() >= 4 + 5 * K,
              "pixel seg bwd: dH like h, scalar loss gradient, the forward's stats");
  TORCH_CHECK(dW.is_contiguous() && dW.numel() == w.numel() && db.is_contiguous() && db.numel() == b.numel(),
              "pixel seg bwd: dW / db like w / b");
  TORCH_CHECK(gout.get_device() == h.get_device() && stats.get_device() == h.get_device() &&
                  dH.get_device() == h.get_device() && dW.get_device() == h.get_device() &&
                  db.get_device() == h.get_device(),
              "pixel seg bwd: every operand on h's device");
  Tensor part = R > 0 ? torch::empty({pio::pixel_ce_blocks(R), (int64_t)K * C + K}, h.options())
                      : torch::zeros({pio::pixel_ce_blocks(R), (int64_t)K * C + K}, h.options());
  pio::pixel_seg_bwd_launch(C, K, f32p(h), f32p(w), f32p(b), labels.data_ptr<int64_t>(), f32p(wts), (float)gamma,
                            (float)ce_weight, (float)dice_weight, (float)eps, f32p(gout), f32p(stats), R,
                            dH.data_ptr<float>(), part.data_ptr<float>(), dW.data_ptr<float>(), db.data_ptr<float>(),
                            stream());
}

// Inference head (pixel_head.hip pixel_predict_kernel): h (R = B·Q, C), one row per query pixel →
// [classes (R) uint8, conf (R) fp32, class_map (B, npix) uint8, confusion partials
// (blocks, K·K) int32 — only with labels].  class_map is cleared on the stream before the launch;
// rows with qvalid False and indices outside [0, npix) leave it untouched.
std::vector<Tensor> pixel_predict(Tensor h, Tensor w, Tensor b, Tensor qidx, Tensor qvalid, int64_t Q, int64_t npix,
                                  OptT labels) {
  CHECK_DT(h, torch::kFloat32); CHECK_DT(w, torch::kFloat32); CHECK_DT(b, torch::kFloat32);
  CHECK_DT(qidx, torch::kInt64); CHECK_DT(qvalid, torch::kBool);
  TORCH_CHECK(h.dim() == 2 && h.is_contiguous() && w.dim() == 2 && w.is_contiguous() && b.is_contiguous() &&
                  qidx.is_contiguous() && qvalid.is_contiguous(), "pixel_predict: contiguous h (R, C), w (K, C)");
  const int C = (int)h.size(1), K = (int)w.size(0);
  const long long R = h.size(0);
  TORCH_CHECK((C == 32 || C == 64 || C == 128) && K >= 2 && K <= 4 && w.size(1) == C && b.numel() == K,
              "pixel_predict: C in {32, 64, 128}, 2 <= K <= 4");
  TORCH_CHECK(Q > 0 && npix > 0 && R % Q == 0 && qidx.numel() == R && qvalid.numel() == R,
              "pixel_predict: R = B * Q rows, one qidx / qvalid entry per row");
  CHECK_CUDA(h);
  TORCH_CHECK(w.get_device() == h.get_device() && b.get_device() == h.get_device() &&
                  qidx.get_device() == h.get_device() && qvalid.get_device() == h.get_device(),
              "pixel_predict: every operand on h's device");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(h.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 == 0,
              "pixel_predict: 16-byte aligned rows");
  const int64_t* lab = nullptr;
  if (labels.has_value()) {
    CHECK_DT(*labels, torch::kInt64);
    TORCH_CHECK(labels->is_contiguous() && labels->numel() == R && labels->get_device() == h.get_device(),
                "pixel_predict: one contiguous label per row, on h's device");
    lab = labels->data_ptr<int64_t>();
  }
  auto u8 = h.options().dtype(torch::kUInt8);
  Tensor classes = torch::empty({R}, u8), conf = torch::empty({R}, h.options());
  Tensor cmap = torch::empty({R / Q, npix}, u8);
  if (cmap.numel() > 0) {
    const hipError_t e = hipMemsetAsync(cmap.data_ptr(), 0, (size_t)cmap.numel(), stream());
    TORCH_CHECK(e == hipSuccess, "pixel_predict: clearing the class map failed: ", hipGetErrorString(e));
  }
  std::vector<Tensor> out{classes, conf, cmap};
  Tensor cpart;
  if (lab != nullptr) {  // every block of the launch stores its whole partial row
    auto i32 = h.options().dtype(torch::kInt32);
    cpart = R > 0 ? torch::empty({pio::pixel_ce_blocks(R), K * K}, i32) : torch::zeros({1, K * K}, i32);
    out.push_back(cpart);
  }
  pio::pixel_predict_launch(C, K, f32p(h), f32p(w), f32p(b), qidx.data_ptr<int64_t>(), qvalid.data_ptr<bool>(), lab, R,
                            Q, npix, classes.data_ptr<uint8_t>(), conf.data_ptr<float>(), cmap.data_ptr<uint8_t>(),
                            lab != nullptr ? cpart.data_ptr<int>() : nullptr, stream());
  checked_sync("pixel_predict");
  return out;
}

// img (B, npix) fp32 → [values (B, cap, 1) fp32, index (B, cap) int64, kmask (B, cap) bool,
// count (B) int32]: the pixels with img != 0 in flat order (pixel_head.hip nonzero_compact);
// cap = 0 only counts.  segs / tile: segments per sample (1..256) and loads per thread and tile
// (4 or 8); 0 picks the measured default (profiles/lartpc_segment.md).
constexpr int kNonzeroSegs = 64, kNonzeroTile = 4;
std::vector<Tensor> nonzero_compact(Tensor img, int64_t cap, int64_t segs, int64_t tile) {
  CHECK_CUDA(img);
  CHECK_DT(img, torch::kFloat32);
  TORCH_CHECK(img.dim() == 2 && img.is_contiguous(), "nonzero_compact: img must be (B, npix) contiguous");
  const int64_t B = img.size(0), npix = img.size(1);
  TORCH_CHECK(B > 0 && B <= 65535 && npix > 0 && npix < (1ll << 31) && cap >= 0, "nonzero_compact: bad shape or capacity");
  TORCH_CHECK(segs >= 0 && segs <= 256 && (tile == 0 || tile == 4 || tile == 8), "nonzero_compact: segs in [0, 256], tile in {0, 4, 8}");
  const int V = tile == 0 ? kNonzeroTile : (int)tile;
  int S = (int)segs;
  if (S == 0) {  // at most kNonzeroSegs segments, none shorter than one tile
    const int64_t tiles = (npix + 256 * V - 1) / (256 * V);
    S = (int)std::min<int64_t>(kNonzeroSegs, tiles);
  }
  Tensor values = torch::empty({B, cap, 1}, img.options()), index = torch::empty({B, cap}, img.options().dtype(torch::kInt64));
  Tensor kmask = torch::empty({B, cap}, img.options().dtype(torch::kBool));
  Tensor count = torch::empty({B}, img.options().dtype(torch::kInt32));
  Tensor segcount;
  if (S > 1) segcount = torch::empty({B, S}, count.options());
  pio::nonzero_compact_launch(f32p(img), (int)B, npix, cap, S, V, S > 1 ? segcount.data_ptr<int>() : nullptr,
                              values.data_ptr<float>(), index.data_ptr<int64_t>(), kmask.data_ptr<bool>(),
                              count.data_ptr<int>(), stream());
  return {values, index, kmask, count};
}

// img (B, H, W) fp32, lab (B, H·W) uint8, words (B) int32 (one dihedral code per sample, read on
// the device) → [values (B, key_cap, 1), index (B, key_cap) int64, kmask (B, key_cap) bool,
// qidx (B, query_cap) int64, qlab (B, query_cap) int64, counts (B, 2) int32] in the flat order of
// the transformed event (lartpc_prep.hip).  wmask: bit c set when class c < ncls is weighted.
// Non-square planes are refused: a transposing word, which the host cannot see, needs H == W.
// Capacities 0 only count.  segs / tile as in nonzero_compact.
std::vector<Tensor> event_compact(Tensor img, Tensor lab, Tensor words, int64_t key_cap, int64_t query_cap, int64_t wmask,
                                  int64_t ncls, int64_t segs, int64_t tile) {
  CHECK_CUDA(img); CHECK_CUDA(lab); CHECK_CUDA(words);
  CHECK_DT(img, torch::kFloat32); CHECK_DT(lab, torch::kUInt8); CHECK_DT(words, torch::kInt32);
  TORCH_CHECK(img.dim() == 3 && img.is_contiguous(), "event_compact: img must be (B, H, W) contiguous");
  const int64_t B = img.size(0), H = img.size(1), W = img.size(2), npix = H * W;
  TORCH_CHECK(H == W, "event_compact: the device path needs square planes (a transposing code needs H == W), got ", H, " x ", W);
  TORCH_CHECK(B > 0 && B <= 65535 && npix > 0 && npix < (1ll << 31) && key_cap >= 0 && query_cap >= 0,
              "event_compact: bad shape or capacity");
  TORCH_CHECK(lab.dim() == 2 && lab.size(0) == B && lab.size(1) == npix && lab.is_contiguous(),
              "event_compact: lab must be (B, H*W) contiguous");
  TORCH_CHECK(words.dim() == 1 && words.size(0) == B && words.is_contiguous(), "event_compact: words must be (B,) contiguous");
  TORCH_CHECK(lab.get_device() == img.get_device() && words.get_device() == img.get_device(),
              "event_compact: img, lab and words must share a device");
  TORCH_CHECK(ncls >= 1 && ncls <= 8 && wmask >= 0 && wmask < (1ll << ncls), "event_compact: at most 8 classes, wmask inside them");
  TORCH_CHECK(segs >= 0 && segs <= 256 && (tile == 0 || tile == 4 || tile == 8), "event_compact: segs in [0, 256], tile in {0, 4, 8}");
  const int V = tile == 0 ? kNonzeroTile : (int)tile;
  int S = (int)segs;
  if (S == 0) S = (int)std::min<int64_t>(kNonzeroSegs, (npix + 256 * V - 1) / (256 * V));
  auto i64 = img.options().dtype(torch::kInt64), i32 = img.options().dtype(torch::kInt32);
  Tensor values = torch::empty({B, key_cap, 1}, img.options()), index = torch::empty({B, key_cap}, i64);
  Tensor kmask = torch::empty({B, key_cap}, img.options().dtype(torch::kBool));
  Tensor qidx = torch::empty({B, query_cap}, i64), qlab = torch::empty({B, query_cap}, i64);
  Tensor counts = torch::empty({B, 2}, i32);
  Tensor segcount;
  if (S > 1) segcount = torch::empty({B, S, 2}, i32);
  pio::EventCompactArgs a{};
  a.img = f32p(img); a.lab = lab.data_ptr<uint8_t>(); a.words = words.data_ptr<int>();
  a.B = (int)B; a.H = (int)H; a.W = (int)W;
  a.kcap = key_cap; a.qcap = query_cap;
  a.wmask = (unsigned)wmask; a.ncls = (int)ncls;
  a.S = S; a.V = V;
  a.segcount = S > 1 ? segcount.data_ptr<int>() : nullptr;
  a.values = values.data_ptr<float>(); a.index = index.data_ptr<int64_t>(); a.kmask = kmask.data_ptr<bool>();
  a.qidx = qidx.data_ptr<int64_t>(); a.qlab = qlab.data_ptr<int64_t>(); a.counts = counts.data_ptr<int>();
  pio::event_compact_launch(a, stream());
  checked_sync("event_compact");
  return {values, index, kmask, qidx, qlab, counts};
}

// ---- the flat-space optimizers (csrc/optim.hip, lamb.hip, ema.hip): one set of argument checks ----
namespace {
bool aligned(const void* q, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(q) & (bytes - 1)) == 0; }

// p, g, m, v: contiguous fp32 device buffers of one size; shadow (optional): contiguous bf16 of that
// size; hyper: contiguous fp32 of at least 8 words on the device.  need_vec: the kernels take float4 /
// uint2 accesses only (adamw falls back to its scalar kernel instead)
struct FlatBufs {
  float *p, *g, *m, *v;
  uint16_t* shadow;
  long long n;
  const float* hyper;
};
FlatBufs flat_bufs(const char* fn, const Tensor& p, const Tensor& g, const Tensor& m, const Tensor& v,
                   const OptT& shadow, const Tensor& hyper, bool need_vec) {
  for (const Tensor* t : {&p, &g, &m, &v, &hyper})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == torch::kFloat32 && t->is_contiguous(), fn,
                ": p, g, m, v and hyper must be contiguous fp32 GPU tensors");
  TORCH_CHECK(p.numel() == g.numel() && p.numel() == m.numel() && p.numel() == v.numel(), fn,
              ": p, g, m, v must have one size");
  TORCH_CHECK(hyper.numel() >= 8, fn, ": hyper of at least 8 floats");
  FlatBufs b{p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(), nullptr, p.numel(),
             hyper.data_ptr<float>()};
  if (shadow.has_value()) {
    TORCH_CHECK(shadow->is_cuda() && shadow->scalar_type() == torch::kBFloat16 && shadow->is_contiguous() &&
                    shadow->numel() == p.numel(),
                fn, ": shadow must be a contiguous bf16 GPU tensor of p's size");
    b.shadow = reinterpret_cast<uint16_t*>(shadow->data_ptr());
  }
  TORCH_CHECK(!need_vec || (aligned(b.p, 16) && aligned(b.g, 16) && aligned(b.m, 16) && aligned(b.v, 16) &&
                            aligned(b.shadow, 8)),
              fn, ": the flat buffers must be 16-byte aligned (the shadow 8-byte)");
  return b;
}

// the step's loss → loss_ring[hyper[7] % n]: both or neither
struct LossRing {
  const float* src;
  float* ring;
  int n;
};
LossRing loss_ring_args(const char* fn, const OptT& loss_src, const OptT& loss_ring) {
  TORCH_CHECK(loss_src.has_value() == loss_ring.has_value(), fn, ": loss_src and loss_ring go together");
  if (!loss_src.has_value()) return {nullptr, nullptr, 1};
  CHECK_DT(*loss_src, torch::kFloat32); CHECK_DT(*loss_ring, torch::kFloat32);
  TORCH_CHECK(loss_src->numel() == 1 && loss_ring->is_contiguous() && loss_ring->numel() >= 1, fn,
              ": scalar loss_src, contiguous loss_ring, hyper[7] = ring slot");
  return {loss_src->data_ptr<float>(), loss_ring->data_ptr<float>(), (int)loss_ring->numel()};
}

// the gradient's sumsq partials, needed (and read) only when clipping
const float* norm_part_arg(const char* fn, double clip, const OptT& norm_part) {
  if (clip <= 0) return nullptr;
  TORCH_CHECK(norm_part.has_value() && norm_part->is_contiguous() && norm_part->numel() >= kSumsqParts &&
                  norm_part->scalar_type() == torch::kFloat32,
              fn, ": clip > 0 needs norm_part (the sumsq partials of the gradient)");
  return norm_part->data_ptr<float>();
}

// the step guard's words (optim_common.h): 8 fp32 on the device, 16-byte aligned; absent = off
const float* guard_arg(const char* fn, const OptT& guard) {
  if (!guard.has_value()) return nullptr;
  TORCH_CHECK(guard->is_cuda() && guard->scalar_type() == torch::kFloat32 && guard->is_contiguous() &&
                  guard->numel() >= 8 && aligned(guard->data_ptr(), 16),
              fn, ": guard must be a contiguous, 16-byte aligned fp32 GPU tensor of 8 words");
  return guard->data_ptr<float>();
}

// chunk_tab (C, 3) int64 = (start, length, tensor) → its pointer; C fits an int
const long long* chunk_tab_arg(const char* fn, const Tensor& chunk_tab) {
  TORCH_CHECK(chunk_tab.is_cuda() && chunk_tab.scalar_type() == torch::kInt64 && chunk_tab.dim() == 2 &&
                  chunk_tab.size(1) == 3 && chunk_tab.is_contiguous() && chunk_tab.size(0) < (int64_t(1) << 31),
              fn, ": chunk_tab must be a contiguous (C, 3) int64 GPU tensor");
  return reinterpret_cast<const long long*>(chunk_tab.data_ptr<int64_t>());
}

// tensor_group (T,) int32 = tensor → group
const int* tensor_group_arg(const char* fn, const Tensor& tensor_group, int64_t T) {
  TORCH_CHECK(tensor_group.is_cuda() && tensor_group.scalar_type() == torch::kInt32 && tensor_group.is_contiguous() &&
                  tensor_group.numel() == T && T < (int64_t(1) << 31),
              fn, ": tensor_group must be a contiguous (T,) int32 GPU tensor");
  return tensor_group.data_ptr<int>();
}
}  // namespace

void adamw(Tensor p, Tensor g, Tensor m, Tensor v, OptT shadow, Tensor hyper, double eps, double wd, double clip,
           double gscale, bool l2, bool zero_grad, OptT loss_src, OptT loss_ring, OptT norm_part, OptT guard) {
  const FlatBufs b = flat_bufs("adamw", p, g, m, v, shadow, hyper, false);
  const LossRing lr = loss_ring_args("adamw", loss_src, loss_ring);
  pio::adamw_launch(b.p, b.g, b.m, b.v, b.shadow, b.n, b.hyper, (float)eps, (float)wd, (float)clip, (float)gscale,
                    l2 ? 1 : 0, zero_grad ? 1 : 0, lr.src, lr.ring, lr.n, norm_part_arg("adamw", clip, norm_part),
                    guard_arg("adamw", guard), stream());
}

// fused LAMB over the flat buffers (csrc/lamb.hip): chunk_tab (C, 3) int64 = (start, length, tensor),
// tensor_tab (T, 2) int32 = (first chunk, chunks), tensor_opt (T, 2) fp32 = (weight decay, adapt);
// partials: >= 2 C fp32 (per-chunk Σw², Σu²), trust: (T,) fp32 (written every step, kept)
void lamb(Tensor p, Tensor g, Tensor m, Tensor v, OptT shadow, Tensor hyper, Tensor chunk_tab, Tensor tensor_tab,
          Tensor tensor_opt, Tensor partials, Tensor trust, double eps, double clip, double gscale, bool zero_grad,
          OptT loss_src, OptT loss_ring, OptT norm_part, OptT tensor_group, OptT guard) {
  const FlatBufs b = flat_bufs("lamb", p, g, m, v, shadow, hyper, true);
  const LossRing lr = loss_ring_args("lamb", loss_src, loss_ring);
  const long long* chunks = chunk_tab_arg("lamb", chunk_tab);
  CHECK_CUDA(tensor_tab); CHECK_CUDA(tensor_opt); CHECK_CUDA(partials); CHECK_CUDA(trust);
  CHECK_DT(tensor_tab, torch::kInt32); CHECK_DT(tensor_opt, torch::kFloat32);
  CHECK_DT(partials, torch::kFloat32); CHECK_DT(trust, torch::kFloat32);
  const int64_t C = chunk_tab.size(0), T = tensor_tab.size(0);
  TORCH_CHECK(tensor_tab.dim() == 2 && tensor_tab.size(1) == 2 && tensor_tab.is_contiguous() &&
                  tensor_opt.is_contiguous() && tensor_opt.dim() == 2 && tensor_opt.size(0) == T &&
                  tensor_opt.size(1) == 2 && T < (int64_t(1) << 31),
              "lamb: tensor_tab (T, 2) int32, tensor_opt (T, 2) fp32, contiguous");
  TORCH_CHECK(partials.is_contiguous() && partials.numel() >= 2 * C && trust.is_contiguous() && trust.numel() >= T,
              "lamb: partials >= 2 C floats, trust >= T floats");
  // per-tensor lr: tensor_group (T,) int32 picks hyper[8 + 4 j]; the group count follows from hyper's width
  const int* tg = nullptr;
  int G = 1;
  if (tensor_group.has_value()) {
    tg = tensor_group_arg("lamb", *tensor_group, T);
    G = (int)((hyper.numel() - 8) / 4);
    TORCH_CHECK(G >= 1 && G <= 8, "lamb: tensor_group needs hyper of 8 + 4 G floats, 1 <= G <= 8");
  }
  pio::lamb_launch(b.p, b.g, b.m, b.v, b.shadow, b.n, b.hyper, chunks, C, tensor_tab.data_ptr<int>(), f32p(tensor_opt),
                   (int)T, partials.data_ptr<float>(), trust.data_ptr<float>(), (float)eps, (float)clip, (float)gscale,
                   zero_grad ? 1 : 0, lr.src, lr.ring, lr.n, norm_part_arg("lamb", clip, norm_part), tg, G,
                   guard_arg("lamb", guard), stream());
}

// AdamW with per-group lr / weight decay / eps (optim.hip adamw_grouped_kernel): chunk_tab (C, 3)
// int64 = (start, length, tensor) as for lamb, tensor_group (T,) int32, hyper = 8 global words + 4 per
// group (lr, weight decay, eps, reserved)
void adamw_grouped(Tensor p, Tensor g, Tensor m, Tensor v, OptT shadow, Tensor hyper, Tensor chunk_tab,
                   Tensor tensor_group, int64_t groups, double clip, double gscale, bool l2, bool zero_grad, OptT loss_src,
                   OptT loss_ring, OptT norm_part, OptT guard) {
  const FlatBufs b = flat_bufs("adamw_grouped", p, g, m, v, shadow, hyper, true);
  const LossRing lr = loss_ring_args("adamw_grouped", loss_src, loss_ring);
  const long long* chunks = chunk_tab_arg("adamw_grouped", chunk_tab);
  const int64_t T = tensor_group.numel();
  const int* tg = tensor_group_arg("adamw_grouped", tensor_group, T);
  TORCH_CHECK(groups >= 1 && groups <= 8 && hyper.numel() >= 8 + 4 * groups,
              "adamw_grouped: 1 <= groups <= 8 and hyper of 8 + 4 * groups floats");
  TORCH_CHECK(pio::adamw_grouped_launch(b.p, b.g, b.m, b.v, b.shadow, b.n, b.hyper, chunks, chunk_tab.size(0), tg, (int)T,
                                        (int)groups, (float)clip, (float)gscale, l2 ? 1 : 0, zero_grad ? 1 : 0, lr.src,
                                        lr.ring, lr.n, norm_part_arg("adamw_grouped", clip, norm_part),
                                        guard_arg("adamw_grouped", guard), stream()) == 0);
}

// the step guard (csrc/health.hip step_guard_kernel): from sumsq's partials and hyper[1] to the 8 guard
// words (read and rewritten: the counters live in them)
void step_guard(Tensor part, Tensor hyper, Tensor guard, double gscale) {
  CHECK_CUDA(part); CHECK_CUDA(hyper); CHECK_DT(part, torch::kFloat32); CHECK_DT(hyper, torch::kFloat32);
  TORCH_CHECK(part.is_contiguous() && part.numel() >= kSumsqParts && hyper.is_contiguous() && hyper.numel() >= 8,
              "step_guard: the sumsq partials (>= 512 floats) and hyper (>= 8 floats), contiguous");
  const float* gp = guard_arg("step_guard", guard);
  TORCH_CHECK(part.get_device() == hyper.get_device() && part.get_device() == guard.get_device(),
              "step_guard: part, hyper and guard on one device");
  pio::step_guard_launch(f32p(part), f32p(hyper), const_cast<float*>(gp), (float)gscale, stream());
}

// per-tensor statistics of the flat gradient and weights (csrc/health.hip): stats (T, 4) fp32 =
// ‖g‖·gscale, ‖w‖, max|g|·gscale, non-finite gradient elements, written when hyper[6] != 0; with a guard
// that flags this step the same rows go to skip_stats.  part: >= 4 C fp32 of scratch.
void tensor_stats(Tensor g, Tensor w, Tensor hyper, Tensor chunk_tab, Tensor tensor_tab, Tensor part, Tensor stats,
                  double gscale, OptT guard, OptT skip_stats) {
  for (const Tensor* t : {&g, &w, &hyper, &part, &stats})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == torch::kFloat32 && t->is_contiguous(),
                "tensor_stats: g, w, hyper, part and stats must be contiguous fp32 GPU tensors");
  const long long* chunks = chunk_tab_arg("tensor_stats", chunk_tab);
  CHECK_CUDA(tensor_tab); CHECK_DT(tensor_tab, torch::kInt32);
  const int64_t C = chunk_tab.size(0), T = tensor_tab.size(0);
  TORCH_CHECK(tensor_tab.dim() == 2 && tensor_tab.size(1) == 2 && tensor_tab.is_contiguous() && T < (int64_t(1) << 31),
              "tensor_stats: tensor_tab (T, 2) int32, contiguous");
  TORCH_CHECK(g.numel() == w.numel() && hyper.numel() >= 8 && part.numel() >= 4 * C && stats.numel() >= 4 * T,
              "tensor_stats: g and w of one size, hyper >= 8, part >= 4 C and stats >= 4 T floats");
  TORCH_CHECK(guard.has_value() == skip_stats.has_value(), "tensor_stats: guard and skip_stats go together");
  float* sp = nullptr;
  if (skip_stats.has_value()) {
    TORCH_CHECK(skip_stats->is_cuda() && skip_stats->scalar_type() == torch::kFloat32 && skip_stats->is_contiguous() &&
                    skip_stats->numel() >= 4 * T && skip_stats->data_ptr() != stats.data_ptr(),
                "tensor_stats: skip_stats must be a second contiguous fp32 GPU tensor of >= 4 T floats");
    sp = skip_stats->data_ptr<float>();
  }
  TORCH_CHECK(aligned(g.data_ptr(), 16) && aligned(w.data_ptr(), 16) && aligned(part.data_ptr(), 16) &&
                  aligned(stats.data_ptr(), 16) && aligned(sp, 16),
              "tensor_stats: the buffers must be 16-byte aligned");
  pio::tensor_stats_launch(f32p(g), f32p(w), g.numel(), f32p(hyper), guard_arg("tensor_stats", guard), chunks, C,
                           tensor_tab.data_ptr<int>(), (int)T, (float)gscale, part.data_ptr<float>(),
                           stats.data_ptr<float>(), sp, stream());
}

// weight EMA over a flat fp32 buffer (csrc/ema.hip): ema ← ema + hyper[5]·(w − ema); hyper[5] = 0
// leaves ema untouched (steps that do not update, inside a static graph)
void ema_update(Tensor ema, Tensor w, Tensor hyper) {
  CHECK_CUDA(ema); CHECK_CUDA(w); CHECK_CUDA(hyper);
  CHECK_DT(ema, torch::kFloat32); CHECK_DT(w, torch::kFloat32); CHECK_DT(hyper, torch::kFloat32);
  TORCH_CHECK(ema.is_contiguous() && w.is_contiguous() && hyper.is_contiguous() && ema.numel() == w.numel() &&
                  ema.get_device() == w.get_device() && ema.get_device() == hyper.get_device(),
              "ema_update: ema and w contiguous fp32 of one size, on the device of hyper");
  TORCH_CHECK(hyper.numel() >= 8, "ema_update: hyper of 8 floats (hyper[5] = 1 - decay)");
  TORCH_CHECK(ema.numel() % 4 == 0, "ema_update: the element count must be a multiple of 4, got ", ema.numel());
  TORCH_CHECK(aligned(ema.data_ptr(), 16) && aligned(w.data_ptr(), 16), "ema_update: the buffers must be 16-byte aligned");
  TORCH_CHECK(ema.numel() == 0 || ema.data_ptr() != w.data_ptr(), "ema_update: ema and w must be different buffers");
  pio::ema_update_launch(ema.data_ptr<float>(), f32p(w), ema.numel(), f32p(hyper), stream());
}

// w ↔ ema in place and (shadow given) shadow ← bf16(new w), one pass; applied twice it restores
// all three buffers bitwise
void ema_swap(Tensor w, Tensor ema, OptT shadow) {
  CHECK_CUDA(w); CHECK_CUDA(ema);
  CHECK_DT(w, torch::kFloat32); CHECK_DT(ema, torch::kFloat32);
  TORCH_CHECK(w.is_contiguous() && ema.is_contiguous() && w.numel() == ema.numel() && w.get_device() == ema.get_device(),
              "ema_swap: w and ema contiguous fp32 of one size on one device");
  TORCH_CHECK(w.numel() % 4 == 0, "ema_swap: the element count must be a multiple of 4, got ", w.numel());
  uint16_t* sp = nullptr;
  if (shadow.has_value()) {
    CHECK_CUDA(*shadow); CHECK_DT(*shadow, torch::kBFloat16);
    TORCH_CHECK(shadow->is_contiguous() && shadow->numel() == w.numel() && shadow->get_device() == w.get_device(),
                "ema_swap: shadow contiguous bf16 of w's size on its device");
    sp = reinterpret_cast<uint16_t*>(shadow->data_ptr());
  }
  TORCH_CHECK(aligned(w.data_ptr(), 16) && aligned(ema.data_ptr(), 16) && aligned(sp, 8),
              "ema_swap: the buffers must be 16-byte aligned (the shadow 8-byte)");
  TORCH_CHECK(w.numel() == 0 || w.data_ptr() != ema.data_ptr(), "ema_swap: w and ema must be different buffers");
  pio::ema_swap_launch(w.data_ptr<float>(), ema.data_ptr<float>(), sp, w.numel(), stream());
}

// self-test of the device cross-lane reductions: (6, 64) = wave_sum, wave_max, half_sum,
// half_max, xor16_sum, xor32_sum of a 64-element fp32 vector
Tensor reduce_probe(Tensor x) {
  TORCH_CHECK(x.is_contiguous() && x.numel() == 64, "reduce_probe takes 64 floats");
  Tensor out = torch::empty({6, 64}, x.options().dtype(torch::kFloat32));
  pio::reduce_probe_launch(f32p(x), out.data_ptr<float>(), stream());
  return out;
}

// grad[:n] += Σ_r rep[r], rep ← 0   (rep: (R, n) contiguous fp32)
void fold_replicas(Tensor grad, Tensor rep) {
  CHECK_DT(grad, torch::kFloat32); CHECK_DT(rep, torch::kFloat32);
  TORCH_CHECK(rep.dim() == 2 && rep.is_contiguous() && grad.is_contiguous() && grad.numel() >= rep.size(1),
              "fold_replicas: rep must be (R, n) contiguous, grad at least n long");
  if (rep.size(1) == 0) return;
  pio::fold_replicas_launch(grad.data_ptr<float>(), rep.data_ptr<float>(), rep.size(1), (int)rep.size(0), stream());
}

// standalone slab job (see make_job)
void slab_reduce(Tensor slab, std::vector<Tensor> dsts, std::vector<int64_t> offs) {
  pio::slab_reduce_launch(make_job(slab, dsts, offs), stream());
}

void cast_bf16(Tensor x, Tensor y) {
  TORCH_CHECK(x.is_contiguous() && y.is_contiguous() && x.numel() == y.numel());
  pio::cast_bf16_launch(f32p(x), reinterpret_cast<uint16_t*>(y.data_ptr()), x.numel(), stream());
}

// factored LN + K/V projection over [pixels ‖ PE] (pe_proj.hip).  pix (R, nc) with R = B·M,
// P (M, O) = (E⊙γ_e)·W_eᵀ, pes/pesq (M), wpg (nc, O), gw/bw (O) → y bf16 (R, O), mean/rstd (R)
std::vector<Tensor> pe_proj_fwd(Tensor pix, Tensor P, Tensor pes, Tensor pesq, Tensor wpg, Tensor gw, Tensor bw,
                                int64_t kin, double eps) {
  for (const Tensor* t : {&pix, &P, &pes, &pesq, &wpg, &gw, &bw}) {
    CHECK_CUDA(*t); CHECK_DT(*t, torch::kFloat32);
    TORCH_CHECK(t->is_contiguous(), "pe_proj_fwd: operands must be contiguous");
  }
  TORCH_CHECK(pix.dim() == 2 && P.dim() == 2, "pe_proj_fwd: pix (R, nc), P (M, O)");
  const long long R = pix.size(0);
  const int nc = (int)pix.size(1), M = (int)P.size(0), O = (int)P.size(1);
  TORCH_CHECK(nc >= 1 && nc <= 4 && O % 4 == 0 && O <= 512 && M > 0 && R % M == 0 && kin > nc,
              "pe_proj_fwd: need 1 <= nc <= 4, O % 4 == 0, O <= 512, R a multiple of M");
  TORCH_CHECK(pes.numel() == M && pesq.numel() == M && wpg.size(0) == nc && wpg.size(1) == O && gw.numel() == O &&
                  bw.numel() == O, "pe_proj_fwd: operand shapes");
  auto y = torch::empty({R, O}, pix.options().dtype(torch::kBFloat16));
  auto mean = torch::empty({R}, pix.options());
  auto rstd = torch::empty({R}, pix.options());
  if (R > 0)
    pio::pe_proj_fwd_launch(f32p(pix), nc, f32p(P), f32p(pes), f32p(pesq), f32p(wpg), f32p(gw), f32p(bw), R, M, O,
                            (int)kin, (float)eps, bfp_mut(y), mean.data_ptr<float>(), rstd.data_ptr<float>(), stream());
  return {y, mean, rstd};
}

// C (M, N) fp32 (bf16 if bf16_out) = A (M, K) bf16 · B (N, K) bf16ᵀ — the factored projection's
// per-step PE GEMM
Tensor pe_gemm(Tensor A, Tensor B, bool bf16_out, int64_t pad_rows) {
  CHECK_CUDA(A); CHECK_DT(A, torch::kBFloat16); CHECK_DT(B, torch::kBFloat16);
  TORCH_CHECK(A.dim() == 2 && B.dim() == 2 && A.is_contiguous() && B.is_contiguous() && A.size(1) == B.size(1),
              "pe_gemm: A (M, K), B (N, K) contiguous");
  const int M = (int)A.size(0), N = (int)B.size(0), K = (int)A.size(1);
  TORCH_CHECK(K % 32 == 0 && N % 128 == 0 && K > 0, "pe_gemm: K a multiple of 32, N a multiple of 128");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(A.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(B.data_ptr()) % 16 == 0,
              "pe_gemm: 16-byte aligned operands");
  TORCH_CHECK(pad_rows >= 0, "pe_gemm: pad_rows >= 0");
  Tensor C = torch::empty({M + pad_rows, N}, A.options().dtype(bf16_out ? torch::kBFloat16 : torch::kFloat32));
  // the zero rows past M (read by prefetches, never used) are written by the GEMM launch itself
  if (M + pad_rows > 0) pio::pe_gemm_launch(bfp(A), bfp(B), C.data_ptr(), bf16_out, M, N, K, (int)(M + pad_rows), stream());
  return C;
}

// weight / LayerNorm gradients of the factored projection, ADDED into the given targets (each
// optional, fp32 contiguous): D (M, O) = Σ_b dY·rσ, part (nblk, (2 + nc)·O) = [ΣdY | ΣdY·μ·rσ |
// ΣdY·x̂_c] partial rows, E (M, Kp) the bf16 PE table, W = [Wa; Wb] (O, kin) as two row blocks
void pe_grads(Tensor D, Tensor part, Tensor E, Tensor Wa, Tensor Wb, Tensor g, Tensor b, int64_t nc, OptT dWa, OptT dWb,
              OptT db, OptT dg, OptT dbeta) {
  for (const Tensor* t : {&D, &part, &Wa, &Wb, &g, &b}) {
    CHECK_CUDA(*t); CHECK_DT(*t, torch::kFloat32);
    TORCH_CHECK(t->is_contiguous(), "pe_grads: contiguous operands");
  }
  CHECK_DT(E, torch::kBFloat16);
  TORCH_CHECK(E.is_contiguous() && E.dim() == 2 && D.dim() == 2 && E.size(0) == D.size(0), "pe_grads: E (M, Kp), D (M, O)");
  const int M = (int)D.size(0), O = (int)D.size(1), Kp = (int)E.size(1), kin = (int)g.numel(), Ch = (int)Wa.size(0);
  const int on = O % 128 == 0 ? 128 : O;  // output columns per workgroup (pe_grads_launch)
  TORCH_CHECK(Kp % 32 == 0 && Kp <= 384 && O % 32 == 0 && on <= 256 && (Kp / 32) * (on / 32) <= 36 && kin <= Kp,
              "pe_grads: Kp a multiple of 32 (≤ 384), O a multiple of 128 or ≤ 256, ≤ 36 output tiles per group");
  TORCH_CHECK(Wa.size(1) == kin && Wb.size(1) == kin && Ch + Wb.size(0) == O && b.numel() == kin, "pe_grads: W shapes");
  TORCH_CHECK(part.size(1) == (2 + nc) * O, "pe_grads: part width");
  auto tgt = [](const OptT& t, int64_t n, const char* name) -> float* {
    if (!t.has_value()) return nullptr;
    CHECK_DT(*t, torch::kFloat32);
    TORCH_CHECK(t->is_contiguous() && t->numel() == n, "pe_grads: target ", name);
    return t->data_ptr<float>();
  };
  pio::PeGradTargets tg{tgt(dWa, (int64_t)Ch * kin, "dWa"), tgt(dWb, (int64_t)(O - Ch) * kin, "dWb"), tgt(db, O, "db"),
                        tgt(dg, kin, "dg"), tgt(dbeta, kin, "dbeta")};
  const int S = pio::pe_grad_splits(M);
  auto f32 = D.options();
  Tensor slab = torch::empty({S, Kp, O}, f32), graw = torch::empty({Kp, O}, f32), tot = torch::empty({(2 + nc) * O}, f32);
  pio::pe_grads_launch(bfp(E), D.data_ptr<float>(), M, Kp, O, part.data_ptr<float>(), (int)part.size(0),
                       slab.data_ptr<float>(), graw.data_ptr<float>(), tot.data_ptr<float>(), Wa.data_ptr<float>(),
                       Wb.data_ptr<float>(), g.data_ptr<float>(), b.data_ptr<float>(), Ch, kin, (int)nc, tg, stream());
}

// W (O, kin) fp32 — or the row blocks W (O1, kin) and W2 (O − O1, kin) of a separate K / V pair,
// never concatenated — γ/β (kin), bias (O) → [Wg (O, Kp) bf16 = W⊙γ on columns [nc, kin) else 0,
// wpg (nc, O) = (W⊙γ)[:, :nc]ᵀ, gw (O) = W·γ, bw (O) = W·β + bias]
std::vector<Tensor> pe_weight_prep(Tensor W, Tensor g, Tensor b, Tensor bias, int64_t nc, int64_t Kp, OptT W2) {
  for (const Tensor* t : {&W, &g, &b, &bias}) {
    CHECK_CUDA(*t); CHECK_DT(*t, torch::kFloat32);
    TORCH_CHECK(t->is_contiguous(), "pe_weight_prep: contiguous operands");
  }
  const int O1 = (int)W.size(0), kin = (int)W.size(1);
  if (W2.has_value()) {
    CHECK_CUDA(*W2); CHECK_DT(*W2, torch::kFloat32);
    TORCH_CHECK(W2->is_contiguous() && W2->dim() == 2 && W2->size(1) == kin, "pe_weight_prep: W2 (O2, kin) contiguous");
  }
  const int O = O1 + (W2.has_value() ? (int)W2->size(0) : 0);
  TORCH_CHECK(g.numel() == kin && b.numel() == kin && bias.numel() == O && nc >= 1 && nc < kin && Kp >= kin,
              "pe_weight_prep: shapes");
  auto f32 = W.options();
  Tensor Wg = torch::empty({O, Kp}, f32.dtype(torch::kBFloat16));
  Tensor wpg = torch::empty({nc, O}, f32), gw = torch::empty({O}, f32), bw = torch::empty({O}, f32);
  Tensor wt = torch::empty({6, O}, f32);  // implicit-K/V generation table (attention_pe.hip)
  TORCH_CHECK(nc <= 4, "pe_weight_prep: at most 4 pixel channels");
  pio::pe_weight_prep_launch(W.data_ptr<float>(), W2.has_value() ? W2->data_ptr<float>() : nullptr, O1,
                             g.data_ptr<float>(), b.data_ptr<float>(), bias.data_ptr<float>(), O,
                             (int)nc, kin, (int)Kp, bfp_mut(Wg), wpg.data_ptr<float>(), gw.data_ptr<float>(),
                             bw.data_ptr<float>(), wt.data_ptr<float>(), stream());
  return {Wg, wpg, gw, bw, wt};
}

// backward pass over dY (R, O): D (M, O) and per-block partials (nblk, (2 + nc)·O) of
// [Σ dY | Σ dY·μ·rσ | Σ dY·x̂_c (c < nc)]
std::vector<Tensor> pe_proj_bwd(Tensor dy, Tensor pix, Tensor mean, Tensor rstd, int64_t M) {
  for (const Tensor* t : {&dy, &pix, &mean, &rstd}) {
    CHECK_CUDA(*t); CHECK_DT(*t, torch::kFloat32);
    TORCH_CHECK(t->is_contiguous(), "pe_proj_bwd: operands must be contiguous");
  }
  TORCH_CHECK(dy.dim() == 2 && pix.dim() == 2 && dy.size(0) == pix.size(0), "pe_proj_bwd: dy (R, O), pix (R, nc)");
  const long long R = dy.size(0);
  const int nc = (int)pix.size(1), O = (int)dy.size(1);
  TORCH_CHECK(M > 0 && R % M == 0 && R / M <= INT32_MAX && nc >= 1 && nc <= 4 && O % 4 == 0 && O <= 512 &&
                  mean.numel() == R && rstd.numel() == R, "pe_proj_bwd: shapes");
  const int nblk = pio::pe_proj_bwd_blocks((int)M);
  auto D = torch::empty({M, O}, dy.options());
  auto part = torch::empty({nblk, (2 + nc) * O}, dy.options());
  pio::pe_proj_bwd_launch(f32p(dy), f32p(pix), nc, f32p(mean), f32p(rstd), (int)(R / M), (int)M, O,
                          D.data_ptr<float>(), part.data_ptr<float>(), stream());
  return {D, part};
}

// encoder cross-attention backward fused with the factored K/V-projection reductions
// (attention_pe.hip): queries (1 | B, Nq ≤ 32, ·), head dim 32, no key mask, no dropout.
// Writes dq (zeroed here) — (Nq, C) summed over the batch for broadcast queries, else (B, Nq, C)
// — and D (M, 2C), part (nkb·bsplit, (2 + nc)·2C), both added onto when accumulate.
// implicit K/V (impl != null): kv / mean / rstd are absent; the factored kernel works from P' (M, 2C)
// bf16, the PE row sums pes / pesq (M) and the per-column table wt (6, 2C) of pe_weight_prep
struct PeImplicit { Tensor P, pes, pesq, wt; double kin, eps; };

// persistent mode of the PE attention backward (attention_pe.hip): one workgroup per CU over
// (key block, head, batch group) items when there are at least as many pairs as CUs
static int pe_bwd_slots(int M, int H, int64_t bsplit) {
  if (g_det || bsplit != 1) return 0;
  int dev = 0, ncu = 256;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
  const int nkb = (M + 255) / 256;
  return (int64_t)nkb * H >= ncu ? ncu : 0;
}

// rows of the `part` buffer the PE attention backward writes for this shape
int64_t attn_bwd_pe_part_rows(int64_t M, int64_t H, int64_t B, int64_t bsplit) {
  const int64_t nkb = (M + 255) / 256;
  const int slots = pe_bwd_slots((int)M, (int)H, bsplit);
  (void)B;
  return slots > 0 ? nkb + slots : nkb * bsplit;
}

static void attn_bwd_pe_impl(Tensor q, const Tensor* kv, Tensor dO, Tensor lse, Tensor delta, const Tensor* mean,
                             const Tensor* rstd, Tensor pix, Tensor dq, Tensor D, Tensor part, int64_t H, double scale,
                             bool accumulate, int64_t bsplit, const PeImplicit* impl, bool dq_zeroed = false,
                             bool d_zeroed = false) {
  for (const Tensor* t : {&q, &dO, &lse, &delta, &pix, &dq, &D, &part}) CHECK_CUDA(*t);
  const int C = (int)(H * 32);
  TORCH_CHECK(q.dim() == 3 && q.stride(2) == 1 && q.size(2) >= C, "q must be (B|1, Nq, >= C) with unit inner stride");
  const int Nq = (int)q.size(1);
  TORCH_CHECK(Nq >= 1 && Nq <= 32, "attn_bwd_pe: at most 32 queries");
  TORCH_CHECK(dO.dim() == 3 && dO.is_contiguous() && dO.size(1) == Nq && dO.size(2) == C, "dO must be (B, Nq, C)");
  const int B = (int)dO.size(0);
  TORCH_CHECK(q.size(0) == 1 || q.size(0) == B, "q batch must be 1 (broadcast) or B");
  const bool qb = q.size(0) == B && B > 1;
  int M;
  if (impl) {
    const Tensor& P = impl->P;
    CHECK_CUDA(P); CHECK_DT(P, torch::kBFloat16);
    M = (int)impl->pes.numel();
    TORCH_CHECK(P.dim() == 2 && P.is_contiguous() && P.size(1) == 2 * C && P.size(0) >= M && M > 0,
                "P must be (>= M, 2C) contiguous, M = pes.numel()");
    for (const Tensor* t : {&impl->pes, &impl->pesq, &impl->wt}) {
      CHECK_CUDA(*t); CHECK_DT(*t, torch::kFloat32);
      TORCH_CHECK(t->is_contiguous(), "attn_bwd_pe: contiguous PE operands");
    }
    TORCH_CHECK(impl->pes.numel() == M && impl->pesq.numel() == M && impl->wt.numel() == 6 * 2 * C,
                "attn_bwd_pe: pes / pesq (M), wt (6, 2C)");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(P.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(impl->wt.data_ptr()) % 16 == 0,
                "attn_bwd_pe: 16-byte aligned P / wt");
  } else {
    CHECK_CUDA(*kv);
    TORCH_CHECK(kv->dim() == 2 && kv->stride(1) == 1 && kv->size(1) >= 2 * C && kv->size(0) % B == 0,
                "kv must be (B*M, >= 2C) rows");
    M = (int)(kv->size(0) / B);
    TORCH_CHECK(kv->stride(0) % 8 == 0 && reinterpret_cast<uintptr_t>(kv->data_ptr()) % 16 == 0,
                "attn_bwd_pe: 16-byte aligned kv rows");
    TORCH_CHECK(mean->numel() == (int64_t)B * M && rstd->numel() == (int64_t)B * M && mean->is_contiguous() &&
                    rstd->is_contiguous(), "row statistics must be (B*M)");
    CHECK_DT(*mean, torch::kFloat32); CHECK_DT(*rstd, torch::kFloat32);
  }
  TORCH_CHECK(q.stride(1) % 8 == 0 && (!qb || q.stride(0) % 8 == 0) && reinterpret_cast<uintptr_t>(q.data_ptr()) % 16 == 0,
              "attn_bwd_pe: 16-byte aligned q rows");
  TORCH_CHECK(pix.dim() == 2 && pix.is_contiguous() && pix.size(0) == (int64_t)B * M && pix.size(1) >= 1 && pix.size(1) <= 4,
              "pix must be (B*M, nc <= 4)");
  const int nc = (int)pix.size(1);
  TORCH_CHECK(lse.is_contiguous() && delta.is_contiguous() && lse.numel() == (int64_t)B * Nq * H && delta.numel() == lse.numel(),
              "lse / delta must be (B, Nq, H)");
  TORCH_CHECK(dq.is_contiguous() && dq.numel() == (int64_t)(qb ? B : 1) * Nq * C,
              "dq must be (Nq, C) for broadcast queries (Σ over the batch), else (B, Nq, C)");
  TORCH_CHECK(D.is_contiguous() && D.size(0) == M && D.size(1) == 2 * C, "D must be (M, 2C) contiguous");
  const int nkb = (M + 255) / 256;
  TORCH_CHECK(bsplit >= 1 && bsplit <= B, "bsplit in [1, B]");
  const int slots = pe_bwd_slots(M, (int)H, bsplit);
  const int64_t prows = slots > 0 ? nkb + slots : (int64_t)nkb * bsplit;
  TORCH_CHECK(part.is_contiguous() && part.size(0) == prows && part.size(1) == (int64_t)(2 + nc) * 2 * C,
              "part must be (attn_bwd_pe_part_rows(M, H, B, bsplit), (2+nc)*2C)");
  for (const Tensor* t : {&lse, &delta, &pix, &dq, &D, &part}) CHECK_DT(*t, torch::kFloat32);
  TORCH_CHECK(!(g_det && bsplit > 1), "deterministic mode: attn_bwd_pe needs bsplit = 1");
  Tensor dq_part;
  if (g_det) dq_part = torch::empty({nkb, dq.numel()}, dq.options());
  else if (!dq_zeroed) dq.zero_();  // dq_zeroed: cleared by the preceding kernel's zero span
  pio::PeBwdArgs a{};
  a.q = bfp(q); a.q_bs = qb ? q.stride(0) : 0; a.q_rs = (int)q.stride(1);
  if (impl) {
    a.P = bfp(impl->P); a.pes = f32p(impl->pes); a.pesq = f32p(impl->pesq); a.wt = f32p(impl->wt);
    a.inv_k = (float)(1.0 / impl->kin); a.eps = (float)impl->eps;
  } else {
    a.kv = bfp(*kv); a.kv_rs = (int)kv->stride(0); a.mean = f32p(*mean); a.rstd = f32p(*rstd);
  }
  a.dO = bfp(dO); a.lse = f32p(lse); a.delta = f32p(delta); a.pix = f32p(pix);
  a.dq = g_det ? dq_part.data_ptr<float>() : dq.data_ptr<float>();
  a.dq_kbs = g_det ? dq.numel() : 0;
  a.D = D.data_ptr<float>(); a.part = part.data_ptr<float>();
  a.B = B; a.H = (int)H; a.Nq = Nq; a.M = M; a.C = C; a.nc = nc;
  a.scale = (float)scale; a.scale_log2 = (float)(scale * 1.4426950408889634);
  a.accumulate = accumulate ? 1 : 0;
  // the split batch groups add into D atomically; d_zeroed: cleared by the preceding kernel's zero span
  if (bsplit > 1 && !accumulate && !d_zeroed) D.zero_();
  Tensor dside, spair;
  if (slots > 0) {
    dside = torch::empty({slots, 256, 64}, D.options());
    spair = torch::empty({slots}, D.options().dtype(torch::kInt32));
    a.nbg = 4; a.nslots = slots; a.Dside = dside.data_ptr<float>(); a.side_pair = spair.data_ptr<int>();
    // slot rows (a side run writes only its head's columns) are cleared by the kernel itself
  }
  pio::attn_bwd_pe_launch(a, nkb, (int)bsplit, stream());
  if (g_det) dq.view({-1}).copy_(dq_part.sum(0));
}

void attn_bwd_pe(Tensor q, Tensor kv, Tensor dO, Tensor lse, Tensor delta, Tensor mean, Tensor rstd, Tensor pix,
                 Tensor dq, Tensor D, Tensor part, int64_t H, double scale, bool accumulate, int64_t bsplit,
                 bool dq_zeroed, bool d_zeroed) {
  attn_bwd_pe_impl(q, &kv, dO, lse, delta, &mean, &rstd, pix, dq, D, part, H, scale, accumulate, bsplit, nullptr,
                   dq_zeroed, d_zeroed);
}

// the same over implicit K/V (attention_pe.hip pe_kv_elem): no (B·M, 2C) K/V tensor, no row statistics
void attn_bwd_pe_implicit(Tensor q, Tensor P, Tensor pes, Tensor pesq, Tensor wt, Tensor dO, Tensor lse, Tensor delta,
                          Tensor pix, Tensor dq, Tensor D, Tensor part, int64_t H, double scale, int64_t kin, double eps,
                          bool accumulate, int64_t bsplit, bool dq_zeroed, bool d_zeroed) {
  PeImplicit im{P, pes, pesq, wt, (double)kin, eps};
  attn_bwd_pe_impl(q, nullptr, dO, lse, delta, nullptr, nullptr, pix, dq, D, part, H, scale, accumulate, bsplit, &im,
                   dq_zeroed, d_zeroed);
}

// encoder cross-attention forward over implicit K/V (attention_pe.hip attn_fwd_pe_kernel): queries
// (1 | B, Nq ≤ 32, ≥ C) bf16, head dim 32, no mask, no dropout; P' (M, 2C) bf16, pix (B·M, nc ≤ 4),
// pes / pesq (M), wt (6, 2C) → O (B, Nq, C) bf16, LSE (B, Nq, H) log2 units.  nsplit key splits.
std::vector<Tensor> attn_fwd_pe(Tensor q, Tensor P, Tensor pix, Tensor pes, Tensor pesq, Tensor wt, int64_t H,
                                double scale, int64_t kin, double eps, int64_t nsplit) {
  for (const Tensor* t : {&q, &P, &pix, &pes, &pesq, &wt}) CHECK_CUDA(*t);
  CHECK_DT(q, torch::kBFloat16); CHECK_DT(P, torch::kBFloat16);
  for (const Tensor* t : {&pix, &pes, &pesq, &wt}) {
    CHECK_DT(*t, torch::kFloat32);
    TORCH_CHECK(t->is_contiguous(), "attn_fwd_pe: contiguous fp32 operands");
  }
  const int C = (int)(H * 32);
  TORCH_CHECK(q.dim() == 3 && q.stride(2) == 1 && q.size(2) >= C && q.stride(1) % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(q.data_ptr()) % 16 == 0, "q must be (B|1, Nq, >= C), 16-byte aligned rows");
  const int Nq = (int)q.size(1);
  TORCH_CHECK(Nq >= 1 && Nq <= 32, "attn_fwd_pe: at most 32 queries");
  const int M = (int)pes.numel();
  TORCH_CHECK(M > 0 && P.dim() == 2 && P.is_contiguous() && P.size(1) == 2 * C && P.size(0) >= M + 64 &&
                  reinterpret_cast<uintptr_t>(P.data_ptr()) % 16 == 0,
              "P must be (M + >= 64 zero pad rows, 2C) contiguous (pe_gemm pad_rows), M = pes.numel()");
  TORCH_CHECK(pix.dim() == 2 && pix.size(0) % M == 0 && pix.size(1) >= 1 && pix.size(1) <= 4, "pix must be (B*M, nc <= 4)");
  const int B = (int)(pix.size(0) / M);
  TORCH_CHECK(q.size(0) == 1 || q.size(0) == B, "q batch must be 1 (broadcast) or B");
  TORCH_CHECK(q.size(0) == 1 || q.stride(0) % 8 == 0, "q batch stride");
  TORCH_CHECK(pesq.numel() == M && wt.numel() == 6 * 2 * C &&
                  reinterpret_cast<uintptr_t>(wt.data_ptr()) % 16 == 0, "attn_fwd_pe: pes / pesq (M), wt (6, 2C)");
  if (nsplit <= 0) {  // one round of waves at the kernel's occupancy on this device
    int dev = 0, ncu = 256;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
    nsplit = pio::attn_fwd_pe_auto_splits(B, (int)H, ncu);
  }
  const int ns = (int)std::max<int64_t>(1, std::min<int64_t>(nsplit, (M + 31) / 32));
  auto o = torch::empty({B, Nq, C}, q.options());
  auto lse = torch::empty({B, Nq, H}, pix.options());
  auto Opart = torch::empty({(int64_t)ns * B * Nq * H * 32}, pix.options());
  auto MLpart = torch::empty({(int64_t)ns * B * Nq * H * 2}, pix.options());
  pio::PeFwdArgs a{};
  a.q = bfp(q); a.q_bs = q.size(0) == 1 ? 0 : q.stride(0); a.q_rs = (int)q.stride(1);
  a.P = bfp(P); a.pix = f32p(pix); a.pes = f32p(pes); a.pesq = f32p(pesq); a.wt = f32p(wt);
  a.Opart = Opart.data_ptr<float>(); a.MLpart = MLpart.data_ptr<float>();
  a.B = B; a.H = (int)H; a.Nq = Nq; a.M = M; a.C = C; a.nc = (int)pix.size(1); a.nsplit = ns;
  a.scale_log2 = (float)(scale * 1.4426950408889634); a.inv_k = (float)(1.0 / (double)kin); a.eps = (float)eps;
  pio::attn_fwd_pe_launch(a, stream());
  pio::attn_combine_launch(a.Opart, a.MLpart, bfp_mut(o), lse.data_ptr<float>(), ns, (long long)B * Nq * H, 32, stream());
  return {o, lse};
}

void set_deterministic(bool on) { g_det = on; }
bool get_deterministic() { return g_det; }

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("set_deterministic", &set_deterministic);
  m.def("check_errors", &check_errors, py::arg("reset") = true);
  m.def("checked_build", &checked_build);
  m.def("get_deterministic", &get_deterministic);
  m.doc() = "Perceiver IO CDNA4 (gfx950) kernels";
  m.def("attn_fwd", &attn_fwd, py::arg("q"), py::arg("k"), py::arg("v"), py::arg("kmask"), py::arg("H"), py::arg("D"),
        py::arg("scale"), py::arg("dropout_p"), py::arg("seed"), py::arg("nsplit"), py::arg("site") = 0);
  m.def("attn_bwd", &attn_bwd, py::arg("q"), py::arg("k"), py::arg("v"), py::arg("kmask"), py::arg("o"), py::arg("dO"),
        py::arg("lse"), py::arg("delta_in"), py::arg("H"), py::arg("D"), py::arg("scale"), py::arg("dropout_p"),
        py::arg("seed"), py::arg("dq_out"), py::arg("dk_out"), py::arg("dv_out"), py::arg("kv_accumulate") = false,
        py::arg("site") = 0, py::arg("dq_zeroed") = false, py::arg("kv_zeroed") = false,
        py::arg("job_slab") = py::none(), py::arg("job_dsts") = std::vector<Tensor>{},
        py::arg("job_offs") = std::vector<int64_t>{});
  m.def("attn_weights", &attn_weights, py::arg("q"), py::arg("k"), py::arg("kmask"), py::arg("lse"), py::arg("H"),
        py::arg("D"), py::arg("scale"), py::arg("want_avg"), py::arg("want_mass"));
  m.def("attn_bwd_zero_plan", &pio::attn_bwd_zero_plan, py::arg("B"), py::arg("H"), py::arg("Nq"), py::arg("Nk"),
        py::arg("D"));
  m.def("ln_linear_fwd", &ln_linear_fwd, py::arg("x"), py::arg("lnw"), py::arg("lnb"), py::arg("eps"), py::arg("w"),
        py::arg("bias"), py::arg("act"), py::arg("res"), py::arg("out_bf16"), py::arg("save_stats"),
        py::arg("pe") = py::none(), py::arg("kin") = -1, py::arg("pe_index") = py::none());
  m.def("post_attn_fwd", &post_attn_fwd, py::arg("o"), py::arg("x"), py::arg("wo"), py::arg("bo"), py::arg("g2"),
        py::arg("be2"), py::arg("eps"), py::arg("w1"), py::arg("b1"), py::arg("w2"), py::arg("b2"),
        py::arg("seed") = py::none(), py::arg("site") = 0, py::arg("p") = 0.0);
  m.def("sa_layer_fwd", &sa_layer_fwd, py::arg("qkv"), py::arg("x"), py::arg("N"), py::arg("scale"), py::arg("wo"),
        py::arg("bo"), py::arg("g2"), py::arg("be2"), py::arg("eps"), py::arg("w1"), py::arg("b1"), py::arg("w2"),
        py::arg("b2"), py::arg("lnw") = py::none(), py::arg("lnb") = py::none(), py::arg("wq") = py::none(),
        py::arg("bq") = py::none(), py::arg("seed") = py::none(), py::arg("site") = 0, py::arg("p") = 0.0);
  m.def("sb_fwd", &sb_fwd, py::arg("x"), py::arg("params"), py::arg("scale"), py::arg("eps"),
        py::arg("pre") = std::vector<Tensor>{}, py::arg("post") = std::vector<Tensor>{});
  m.def("sb_bwd", &sb_bwd, py::arg("dz"), py::arg("x0"), py::arg("saved"), py::arg("params"),
        py::arg("scale"), py::arg("eps"), py::arg("pre") = std::vector<Tensor>{},
        py::arg("pre_saved") = std::vector<Tensor>{}, py::arg("zero_out") = py::none(),
        py::arg("post") = std::vector<Tensor>{}, py::arg("post_io") = std::vector<Tensor>{});
  m.def("sb_wgrad", &sb_wgrad, py::arg("jobs"), py::arg("job_slab") = py::none(),
        py::arg("job_dsts") = std::vector<Tensor>(), py::arg("job_offs") = std::vector<int64_t>());
  m.def("post_attn_ln_linear_fwd", &post_attn_ln_linear_fwd, py::arg("o"), py::arg("x"), py::arg("wo"), py::arg("bo"),
        py::arg("g2"), py::arg("be2"), py::arg("eps"), py::arg("w1"), py::arg("b1"), py::arg("w2"), py::arg("b2"),
        py::arg("lnw"), py::arg("lnb"), py::arg("wq"), py::arg("bq"), py::arg("seed") = py::none(),
        py::arg("site") = 0, py::arg("p") = 0.0);
  m.def("ln_linear_post_attn_bwd", &ln_linear_post_attn_bwd, py::arg("g"), py::arg("wq"), py::arg("x"),
        py::arg("mean1"), py::arg("rstd1"), py::arg("lnw"), py::arg("lnb"), py::arg("dres"), py::arg("ll_grads"),
        py::arg("y"), py::arg("m2"), py::arg("r2"), py::arg("u"), py::arg("o"), py::arg("wo"), py::arg("w1"),
        py::arg("w2"), py::arg("g2"), py::arg("be2"), py::arg("H"), py::arg("pa_grads"),
        py::arg("job_slab") = py::none(), py::arg("job_dsts") = std::vector<Tensor>(),
        py::arg("job_offs") = std::vector<int64_t>(), py::arg("seed") = py::none(), py::arg("site") = 0,
        py::arg("p") = 0.0, py::arg("zero_out") = py::none(), py::arg("att_qkv") = py::none(),
        py::arg("att_lse") = py::none(), py::arg("att_out") = py::none(), py::arg("att_scale") = 0.0);
  m.def("post_attn_bwd", &post_attn_bwd, py::arg("dz"), py::arg("y"), py::arg("m2"), py::arg("r2"), py::arg("u"),
        py::arg("o"), py::arg("wo"), py::arg("w1"), py::arg("w2"), py::arg("g2"), py::arg("be2"), py::arg("H"),
        py::arg("grads"), py::arg("slab") = false, py::arg("job_slab") = py::none(),
        py::arg("job_dsts") = std::vector<Tensor>(), py::arg("job_offs") = std::vector<int64_t>(),
        py::arg("seed") = py::none(), py::arg("site") = 0, py::arg("p") = 0.0, py::arg("zero_out") = py::none());
  m.def("ln_linear_bwd", &ln_linear_bwd, py::arg("g"), py::arg("w"), py::arg("x"), py::arg("mean"), py::arg("rstd"),
        py::arg("lnw"), py::arg("lnb"), py::arg("dres"), py::arg("need_dx"), py::arg("dlnw"), py::arg("dlnb"),
        py::arg("dW"), py::arg("db"), py::arg("pe") = py::none(), py::arg("kin") = -1, py::arg("slab") = false,
        py::arg("job_slab") = py::none(), py::arg("job_dsts") = std::vector<Tensor>(),
        py::arg("job_offs") = std::vector<int64_t>(), py::arg("dx_out") = py::none(), py::arg("pe_index") = py::none());
  m.def("text_kv_fwd", &text_kv_fwd, py::arg("ids"), py::arg("E"), py::arg("P"), py::arg("scale"), py::arg("eps"),
        py::arg("la"), py::arg("lb"));
  m.def("text_kv_bwd", &text_kv_bwd, py::arg("ga"), py::arg("gb"), py::arg("x"), py::arg("mean"), py::arg("rstd"),
        py::arg("la"), py::arg("lb"), py::arg("grads"), py::arg("slab") = false, py::arg("job_slab") = py::none(),
        py::arg("job_dsts") = std::vector<Tensor>(), py::arg("job_offs") = std::vector<int64_t>());
  m.def("wgrad", &wgrad, py::arg("g"), py::arg("a"), py::arg("amode"), py::arg("mean"), py::arg("rstd"), py::arg("lnw"),
        py::arg("lnb"), py::arg("rows_per_wg"), py::arg("dW"), py::arg("db"), py::arg("pe") = py::none(),
        py::arg("kin") = -1, py::arg("pe_index") = py::none());
  m.def("mlm_select", &mlm_select, py::arg("labels"), py::arg("cap"), py::arg("gcap"), py::arg("sticky") = py::none(),
        py::arg("queries") = py::none());
  m.def("index_add_rows", &index_add_rows);
  m.def("gather_rows", &gather_rows, py::arg("src"), py::arg("idx"));
  m.def("batch_sum2", &batch_sum2, py::arg("a"), py::arg("b"), py::arg("ob_acc") = py::none());
  m.def("pixel_ce_fwd", &pixel_ce_fwd);
  m.def("pixel_ce_bwd", &pixel_ce_bwd);
  m.def("pixel_seg_fwd", &pixel_seg_fwd);
  m.def("pixel_seg_bwd", &pixel_seg_bwd);
  m.def("pixel_predict", &pixel_predict, py::arg("h"), py::arg("w"), py::arg("b"), py::arg("qidx"), py::arg("qvalid"),
        py::arg("Q"), py::arg("npix"), py::arg("labels") = py::none());
  m.def("nonzero_compact", &nonzero_compact, py::arg("img"), py::arg("cap"), py::arg("segs") = 0, py::arg("tile") = 0);
  m.def("event_compact", &event_compact, py::arg("img"), py::arg("lab"), py::arg("words"), py::arg("key_cap"),
        py::arg("query_cap"), py::arg("wmask"), py::arg("ncls"), py::arg("segs") = 0, py::arg("tile") = 0);
  m.def("stage_step", &stage_step, py::arg("dsts"), py::arg("srcs"), py::arg("hyper_dst") = py::none(),
        py::arg("hyper") = std::vector<double>{}, py::arg("seed_dst") = py::none(),
        py::arg("seeds") = std::vector<int64_t>{});
  m.def("ce_fwd", &ce_fwd, py::arg("h"), py::arg("idx"), py::arg("labels"), py::arg("w"), py::arg("bias"),
        py::arg("count"), py::arg("zero_out") = py::none(), py::arg("count_labels") = false);
  m.def("ce_bwd", &ce_bwd, py::arg("h"), py::arg("labels"), py::arg("w"), py::arg("bias"),
        py::arg("lse"), py::arg("gout"), py::arg("count"), py::arg("dH"), py::arg("dW"), py::arg("db"),
        py::arg("accumulate"), py::arg("rowmap") = py::none(), py::arg("slab") = false, py::arg("u") = py::none(),
        py::arg("u_ml") = py::none());
  m.def("vocab_topk", &vocab_topk, py::arg("h"), py::arg("idx"), py::arg("w"), py::arg("bias"), py::arg("k"));
  m.def("soft_ce_fwd", &soft_ce_fwd, py::arg("h"), py::arg("label_a"), py::arg("label_b"), py::arg("lam"), py::arg("w"),
        py::arg("bias"), py::arg("eps"));
  m.def("soft_ce_bwd", &soft_ce_bwd, py::arg("hs"), py::arg("label_a"), py::arg("label_b"), py::arg("lam"), py::arg("w"),
        py::arg("bias"), py::arg("eps"), py::arg("lse"), py::arg("gout"), py::arg("count"), py::arg("dH"), py::arg("dW"),
        py::arg("db"), py::arg("accumulate"));
  m.def("batch_mix", &batch_mix, py::arg("x"), py::arg("y"), py::arg("mix"));
  m.def("batch_augment", &batch_augment, py::arg("src"), py::arg("params"), py::arg("mean"), py::arg("std"),
        py::arg("out_h"), py::arg("out_w"));
  m.def("rand_augment", &rand_augment, py::arg("src"), py::arg("words"), py::arg("fill") = 0);
  m.def("embed_fwd", &embed_fwd);
  m.def("embed_bwd", &embed_bwd, py::arg("ids"), py::arg("g"), py::arg("dE"), py::arg("dP"), py::arg("scale"),
        py::arg("job_slab") = py::none(), py::arg("job_dsts") = std::vector<Tensor>(),
        py::arg("job_offs") = std::vector<int64_t>());
  m.def("text_mask", &text_mask, py::arg("x"), py::arg("pad"), py::arg("state"), py::arg("unk"), py::arg("mask"),
        py::arg("p"), py::arg("lo"), py::arg("hi"), py::arg("advance") = true);
  m.def("text_mask_words", &text_mask_words, py::arg("x"), py::arg("pad"), py::arg("state"), py::arg("table"),
        py::arg("unk"), py::arg("mask"), py::arg("p"), py::arg("lo"), py::arg("hi"), py::arg("advance") = true);
  m.def("sumsq", &sumsq);
  m.def("adamw", &adamw, py::arg("p"), py::arg("g"), py::arg("m"), py::arg("v"), py::arg("shadow"), py::arg("hyper"),
        py::arg("eps"), py::arg("wd"), py::arg("clip"), py::arg("gscale"), py::arg("l2") = false,
        py::arg("zero_grad") = false, py::arg("loss_src") = py::none(), py::arg("loss_ring") = py::none(),
        py::arg("norm_part") = py::none(), py::arg("guard") = py::none());
  m.def("lamb", &lamb, py::arg("p"), py::arg("g"), py::arg("m"), py::arg("v"), py::arg("shadow"), py::arg("hyper"),
        py::arg("chunk_tab"), py::arg("tensor_tab"), py::arg("tensor_opt"), py::arg("partials"), py::arg("trust"),
        py::arg("eps"), py::arg("clip"), py::arg("gscale"), py::arg("zero_grad") = false,
        py::arg("loss_src") = py::none(), py::arg("loss_ring") = py::none(), py::arg("norm_part") = py::none(),
        py::arg("tensor_group") = py::none(), py::arg("guard") = py::none());
  m.def("adamw_grouped", &adamw_grouped, py::arg("p"), py::arg("g"), py::arg("m"), py::arg("v"), py::arg("shadow"),
        py::arg("hyper"), py::arg("chunk_tab"), py::arg("tensor_group"), py::arg("groups"), py::arg("clip"),
        py::arg("gscale"), py::arg("l2") = false, py::arg("zero_grad") = false, py::arg("loss_src") = py::none(),
        py::arg("loss_ring") = py::none(), py::arg("norm_part") = py::none(), py::arg("guard") = py::none());
  m.def("step_guard", &step_guard, py::arg("part"), py::arg("hyper"), py::arg("guard"), py::arg("gscale"));
  m.def("tensor_stats", &tensor_stats, py::arg("g"), py::arg("w"), py::arg("hyper"), py::arg("chunk_tab"),
        py::arg("tensor_tab"), py::arg("part"), py::arg("stats"), py::arg("gscale"), py::arg("guard") = py::none(),
        py::arg("skip_stats") = py::none());
  m.attr("LAMB_CHUNK") = pio::lamb_chunk_elems();
  m.def("ema_update", &ema_update, py::arg("ema"), py::arg("w"), py::arg("hyper"));
  m.def("ema_swap", &ema_swap, py::arg("w"), py::arg("ema"), py::arg("shadow") = py::none());
  m.attr("EMA_PASS_ELEMS") = pio::ema_pass_elems();
  m.def("cast_bf16", &cast_bf16);
  m.def("reduce_probe", &reduce_probe);
  m.def("fold_replicas", &fold_replicas);
  m.def("slab_reduce", &slab_reduce);
  m.def("pe_proj_fwd", &pe_proj_fwd);
  m.def("pe_gemm", &pe_gemm, py::arg("A"), py::arg("B"), py::arg("bf16_out") = false, py::arg("pad_rows") = 0);
  m.def("attn_fwd_pe", &attn_fwd_pe);
  m.def("sa_block_fwd", &sa_block_fwd, py::arg("qkv0"), py::arg("x0"), py::arg("N"), py::arg("scale"), py::arg("eps"),
        py::arg("wo"), py::arg("bo"), py::arg("g2"), py::arg("be2"), py::arg("w1"), py::arg("b1"), py::arg("w2"),
        py::arg("b2"), py::arg("lnw"), py::arg("lnb"), py::arg("wq"), py::arg("bq"), py::arg("seed") = py::none(),
        py::arg("p") = 0.0);
  m.def("persist_errors", &persist_errors, py::arg("reset") = true);
  m.def("persist_set_spin_limit", [](int64_t n) { pio::persist_set_spin_limit((unsigned)n); }, py::arg("n"));
  m.def("attn_bwd_pe_part_rows", &attn_bwd_pe_part_rows);
  m.def("attn_bwd_pe_implicit", &attn_bwd_pe_implicit, py::arg("q"), py::arg("P"), py::arg("pes"), py::arg("pesq"),
        py::arg("wt"), py::arg("dO"), py::arg("lse"), py::arg("delta"), py::arg("pix"), py::arg("dq"), py::arg("D"),
        py::arg("part"), py::arg("H"), py::arg("scale"), py::arg("kin"), py::arg("eps"), py::arg("accumulate"),
        py::arg("bsplit"), py::arg("dq_zeroed") = false, py::arg("d_zeroed") = false);
  m.def("pe_weight_prep", &pe_weight_prep, py::arg("W"), py::arg("g"), py::arg("b"), py::arg("bias"), py::arg("nc"),
        py::arg("Kp"), py::arg("W2") = py::none());
  m.def("pe_grads", &pe_grads);
  m.def("pe_proj_bwd", &pe_proj_bwd);
  m.def("attn_bwd_pe", &attn_bwd_pe, py::arg("q"), py::arg("kv"), py::arg("dO"), py::arg("lse"), py::arg("delta"),
        py::arg("mean"), py::arg("rstd"), py::arg("pix"), py::arg("dq"), py::arg("D"), py::arg("part"), py::arg("H"),
        py::arg("scale"), py::arg("accumulate"), py::arg("bsplit"), py::arg("dq_zeroed") = false,
        py::arg("d_zeroed") = false);
  m.attr("arch") = "gfx950";
}
