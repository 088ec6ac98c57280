// Flash attention forward / backward (attention.hip), with one optional mask kind: dropout on the probabilities, a
// document mask or a span mask. Which kinds combine with which shapes, and which kernels run, is flash_plan's to say.
#include "binding/common.h"

namespace k8s_amd::binding {
namespace {

void check_attn_operand(const Tensor& t, const char* name, long D) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  check_dtype(t, at::kBFloat16, name);
  TORCH_CHECK(t.dim() == 4, name, " must be [B, S, H, D]");
  TORCH_CHECK(t.size(3) == D && t.stride(3) == 1, name, " must have a contiguous head dim of ", D);
  for (int i = 0; i < 3; ++i) TORCH_CHECK(t.stride(i) % 8 == 0, name, " strides must be multiples of 8 elements");
  check_aligned(t, name);
}
const int* kv_lens_ptr(const OptTensor& kv_lens, long B) {
  if (!kv_lens) return nullptr;
  TORCH_CHECK(kv_lens->is_cuda() && kv_lens->scalar_type() == at::kInt && kv_lens->is_contiguous() &&
                  kv_lens->numel() == B, "kv_lens must be an int32 GPU tensor of length B");
  return kv_lens->data_ptr<int>();
}

// The mask kind of a call: drop_state, or doc_lo / doc_hi, or span_lo / span_hi (a pair: both or neither; int32
// [B, Sq] tables the kernels clamp before use). Only what is about the tensors is checked here.
template <class Args>
void fill_mask(Args& a, const OptTensor& drop_state, int64_t drop_thr, double drop_scale, int64_t drop_site,
               const OptTensor& doc_lo, const OptTensor& doc_hi, const OptTensor& span_lo, const OptTensor& span_hi,
               int64_t span_tile) {
  const bool doc = doc_lo || doc_hi, span = span_lo || span_hi;
  TORCH_CHECK((int)doc + (int)span + (int)drop_state.has_value() <= 1,
              "dropout, a document mask and a span mask cannot be combined");
  TORCH_CHECK(span_tile >= 0 && span_tile <= 128, "span_tile must be 0, 64 or 128, got ", span_tile);
  a.span_tile = (int)span_tile;
  if (drop_state) {
    a.mask = AttnMask::Drop;
    a.drop = drop_args(*drop_state, drop_thr, drop_scale, drop_site);
  }
  if (!doc && !span) return;
  const OptTensor &lo = doc ? doc_lo : span_lo, &hi = doc ? doc_hi : span_hi;
  const char* names = doc ? "doc_lo / doc_hi" : "span_lo / span_hi";
  TORCH_CHECK(lo && hi, names, " must be given together");
  for (const Tensor* t : {&*lo, &*hi})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kInt && t->is_contiguous() && t->dim() == 2 &&
                    t->size(0) == a.B && t->size(1) == a.Sq, names, " must be contiguous int32 GPU tensors [B, Sq]");
  a.mask = doc ? AttnMask::Doc : AttnMask::Span;
  a.mask_lo = lo->data_ptr<int>();
  a.mask_hi = hi->data_ptr<int>();
}

// what AttnFwdArgs and AttnBwdArgs share: q / k / v [B, S, H, D] with their strides, the shape, the softmax scale and
// kv_lens. Returns the head dim D.
template <class Args>
long fill_qkv(Args& a, const Tensor& q, const Tensor& k, const Tensor& v, bool causal, const OptTensor& kv_lens,
              double scale) {
  TORCH_CHECK(q.dim() == 4 && (q.size(3) == 64 || q.size(3) == 128), "head dim must be 64 or 128");
  const long D = q.size(3);
  check_attn_operand(q, "q", D); check_attn_operand(k, "k", D); check_attn_operand(v, "v", D);
  a.B = q.size(0); a.Sq = q.size(1); a.Hq = q.size(2); a.Sk = k.size(1); a.Hkv = k.size(2); a.causal = causal;
  TORCH_CHECK(k.size(0) == a.B && v.size(0) == a.B && v.size(1) == a.Sk && v.size(2) == a.Hkv, "k/v shape mismatch");
  TORCH_CHECK(a.Hkv > 0 && a.Hq % a.Hkv == 0, "Hq must be a multiple of Hkv");
  TORCH_CHECK(a.Sq > 0 && a.Sk > 0, "empty sequence");
  a.kv_lens = kv_lens_ptr(kv_lens, a.B);
  a.q = cbf(q); a.k = cbf(k); a.v = cbf(v);
  a.sqb = q.stride(0); a.sqs = q.stride(1); a.sqh = q.stride(2);
  a.skb = k.stride(0); a.sks = k.stride(1); a.skh = k.stride(2);
  a.svb = v.stride(0); a.svs = v.stride(1); a.svh = v.stride(2);
  a.scale_log2 = (float)(scale * 1.4426950408889634);
  return D;
}

std::vector<Tensor> flash_fwd(Tensor q, Tensor k, Tensor v, bool causal, OptTensor kv_lens, double scale,
                              OptTensor drop_state, int64_t drop_thr, double drop_scale, int64_t drop_site,
                              OptTensor doc_lo, OptTensor doc_hi, OptTensor span_lo, OptTensor span_hi,
                              int64_t span_tile) {
  AttnFwdArgs a;
  const long D = fill_qkv(a, q, k, v, causal, kv_lens, scale);
  const long B = a.B, Sq = a.Sq, Hq = a.Hq;
  fill_mask(a, drop_state, drop_thr, drop_scale, drop_site, doc_lo, doc_hi, span_lo, span_hi, span_tile);
  auto o = torch::empty({B, Sq, Hq, D}, q.options());
  const long ld = (Sq + 127) / 128 * 128;  // padded rows: the backward stages 64/128-query slices with 16-B copies
  auto lse = torch::empty({B, Hq, ld}, q.options().dtype(at::kFloat));
  a.o = bf(o); a.lse = f32(lse); a.lse_ld = ld;
  a.sob = o.stride(0); a.sos = o.stride(1); a.soh = o.stride(2);
  launch_flash_fwd(a, (int)D, cur_stream());  // (throws the plan's reason for a shape or combination it does not take)
  return {o, lse};
}

// dq / dk / dv are new contiguous tensors, or -- with `dqkv` given -- views into that [B*S, (Hq + 2*Hkv) * D]
// buffer laid out like the packed QKV projection q / k / v were sliced from (q at column 0, k at Hq*D, v at
// (Hq + Hkv)*D): the fused projection's gradient is written in place, no concatenation afterwards.
std::vector<Tensor> flash_bwd(Tensor dO, Tensor q, Tensor k, Tensor v, Tensor o, Tensor lse, bool causal,
                              OptTensor kv_lens, double scale, OptTensor dqkv, OptTensor dbias, OptTensor drop_state,
                              int64_t drop_thr, double drop_scale, int64_t drop_site, OptTensor doc_lo,
                              OptTensor doc_hi, OptTensor span_lo, OptTensor span_hi, int64_t span_tile) {
  AttnBwdArgs a;
  const long D = fill_qkv(a, q, k, v, causal, kv_lens, scale);
  const long B = a.B, Sq = a.Sq, Hq = a.Hq, Sk = a.Sk, Hkv = a.Hkv;
  fill_mask(a, drop_state, drop_thr, drop_scale, drop_site, doc_lo, doc_hi, span_lo, span_hi, span_tile);
  check_attn_operand(o, "o", D); check_attn_operand(dO, "dO", D);
  TORCH_CHECK(dO.sizes() == q.sizes() && o.sizes() == q.sizes(), "dO / o must match q");
  check_cuda(lse, "lse"); check_dtype(lse, at::kFloat, "lse");
  const long ld = (Sq + 127) / 128 * 128;
  TORCH_CHECK(lse.dim() == 3 && lse.size(0) == B && lse.size(1) == Hq && lse.size(2) == ld,
              "lse must be the [B, Hq, round_up(Sq, 128)] tensor flash_fwd returned");
  const long Wp = (Hq + 2 * Hkv) * D;  // the packed QKV projection's width
  Tensor dq, dk, dv;
  if (dqkv) {
    TORCH_CHECK(Sq == Sk, "packed QKV gradient needs self-attention (Sq == Sk)");
    check_cuda(*dqkv, "dqkv"); check_dtype(*dqkv, at::kBFloat16, "dqkv");
    TORCH_CHECK(dqkv->numel() == B * Sq * Wp, "dqkv must be contiguous [B*S, (Hq+2*Hkv)*D]");
    auto g = dqkv->view({B, Sq, Hq + 2 * Hkv, D});
    dq = g.narrow(2, 0, Hq);
    dk = g.narrow(2, Hq, Hkv);
    dv = g.narrow(2, Hq + Hkv, Hkv);
  } else {
    dq = torch::empty({B, Sq, Hq, D}, q.options());
    dk = torch::empty({B, Sk, Hkv, D}, q.options());
    dv = torch::empty({B, Sk, Hkv, D}, q.options());
  }
  if (dbias) {  // the packed projection's bias gradient from the one-block kernel's column partials
    TORCH_CHECK(dqkv, "dbias needs the packed gradient dqkv");
    check_channel_f32(*dbias, Wp, "dbias");
  }
  auto delta = torch::empty({B, Hq, ld}, q.options().dtype(at::kFloat));
  a.dO = cbf(dO); a.lse = f32(lse); a.lse_ld = ld; a.delta = f32(delta);
  a.dq = bf(dq); a.dk = bf(dk); a.dv = bf(dv);
  a.sdb = dO.stride(0); a.sds = dO.stride(1); a.sdh = dO.stride(2);
  a.sgqb = dq.stride(0); a.sgqs = dq.stride(1); a.sgqh = dq.stride(2);
  a.sgkb = dk.stride(0); a.sgks = dk.stride(1); a.sgkh = dk.stride(2);
  a.sgvb = dv.stride(0); a.sgvs = dv.stride(1); a.sgvh = dv.stride(2);
  a.scale = (float)scale;
  // the workspaces the plan asks for (the launcher throws its reason when it does not take the call)
  const FlashPlan p = k8s_amd::flash_plan(a, (int)D, o.stride(1), dbias.has_value());
  Tensor dkv_ws, rowkey, cpart;
  if (p.ok) {
    a.dkv_split = p.bwd.dkv_split;
    if (p.bwd.dkv_split > 1) {
      dkv_ws = torch::empty({a.dkv_split, 2, B, Hkv, Sk, D}, q.options().dtype(at::kFloat));
      a.dkv_ws = f32(dkv_ws);
    }
    if (p.bwd.needs_rowkey) {  // rows padded like delta's
      rowkey = torch::empty({B, Hq, ld}, q.options().dtype(at::kInt));
      a.rowkey = reinterpret_cast<uint32_t*>(rowkey.data_ptr<int>());
    }
  }
  if (dbias) {
    cpart = torch::empty({B, Wp}, q.options().dtype(at::kFloat));
    a.cpart = f32(cpart);
    a.cpart_ld = (int)Wp;
  }
  launch_flash_bwd(a, (int)D, cbf(o), o.stride(0), o.stride(1), o.stride(2), cur_stream());
  if (dbias) launch_colsum_fold(a.cpart, (int)B, a.cpart_ld, f32(*dbias), false, cur_stream());
  return {dq, dk, dv};
}

AttnMask mask_kind(const std::string& s) {
  TORCH_CHECK(s == "plain" || s == "drop" || s == "doc" || s == "span", "mask must be plain, drop, doc or span; got ", s);
  return s == "plain" ? AttnMask::Plain : s == "drop" ? AttnMask::Drop : s == "doc" ? AttnMask::Doc : AttnMask::Span;
}

py::dict flash_plan(int64_t D, int64_t B, int64_t Sq, int64_t Sk, int64_t Hq, int64_t Hkv, bool causal,
                    bool has_kv_lens, const std::string& mask, int64_t span_tile, int64_t max_token_stride,
                    bool want_dbias) {
  const int tile = (int)std::min<int64_t>(std::max<int64_t>(span_tile, -1), 129);  // (outside 0 / 64 / 128: not ok)
  const FlashPlan p = k8s_amd::flash_plan((int)D, B, Sq, Sk, Hq, Hkv, causal, has_kv_lens, mask_kind(mask), tile,
                                          max_token_stride, want_dbias);
  py::dict fwd, bwd, d;
  fwd["tile"] = p.fwd.tile; fwd["nb"] = p.fwd.nb;
  bwd["one_block"] = p.bwd.one_block; bwd["tile"] = p.bwd.tile; bwd["qs"] = p.bwd.qs;
  bwd["dkv_split"] = p.bwd.dkv_split; bwd["needs_rowkey"] = p.bwd.needs_rowkey;
  d["ok"] = p.ok; d["reason"] = p.reason; d["fwd"] = fwd; d["bwd"] = bwd;
  return d;
}

// the plan of a bare shape, for the predicates below
FlashPlan shape_plan(int64_t D, int64_t B, int64_t Sq, int64_t Sk, int64_t Hq, int64_t Hkv, bool causal, AttnMask mask,
                     int64_t max_token_stride = 0) {
  return k8s_amd::flash_plan((int)D, B, Sq, Sk, Hq, Hkv, causal, false, mask, 0, max_token_stride, false);
}

}  // namespace

void bind_attention(pybind11::module_& m) {
  m.def("flash_fwd", &flash_fwd, "q"_a, "k"_a, "v"_a, "causal"_a, "kv_lens"_a, "scale"_a, "drop_state"_a = py::none(),
        "drop_thr"_a = 0, "drop_scale"_a = 1.0, "drop_site"_a = 0, "doc_lo"_a = py::none(), "doc_hi"_a = py::none(),
        "span_lo"_a = py::none(), "span_hi"_a = py::none(), "span_tile"_a = 0);
  m.def("flash_bwd", &flash_bwd, "dO"_a, "q"_a, "k"_a, "v"_a, "o"_a, "lse"_a, "causal"_a, "kv_lens"_a, "scale"_a,
        "dqkv"_a = py::none(), "dbias"_a = py::none(), "drop_state"_a = py::none(), "drop_thr"_a = 0,
        "drop_scale"_a = 1.0, "drop_site"_a = 0, "doc_lo"_a = py::none(), "doc_hi"_a = py::none(),
        "span_lo"_a = py::none(), "span_hi"_a = py::none(), "span_tile"_a = 0);
  m.def("flash_plan", &flash_plan, "D"_a, "B"_a, "Sq"_a, "Sk"_a, "Hq"_a, "Hkv"_a, "causal"_a = false,
        "has_kv_lens"_a = false, "mask"_a = "plain", "span_tile"_a = 0, "max_token_stride"_a = 0,
        "want_dbias"_a = false,
        "whether flash_fwd / flash_bwd take a call (ok, reason) and which kernels run: fwd {tile, nb}, bwd {one_block, "
        "tile, qs, dkv_split, needs_rowkey}; mask is plain, drop, doc or span");
  // ---- views of the plan
  m.def("flash_span_ok", [](int64_t D, int64_t B, int64_t Sq, int64_t Sk, int64_t Hq, int64_t max_token_stride) {
          return shape_plan(D, B, Sq, Sk, Hq, Hq, false, AttnMask::Span, max_token_stride).ok;
        }, "whether the span forms of flash_fwd / flash_bwd index this shape (D = 64, Sq == Sk < 2^24, B * Hq * Sq < 2^31, "
           "token strides < 2^24)");
  m.def("flash_span_tile", [](int64_t S) { return shape_plan(64, 1, S, S, 1, 1, false, AttnMask::Span).fwd.tile; },
        "keys per tile the span forms take by default");
  m.def("flash_bwd_one_block", [](int64_t D, int64_t Sq, int64_t Sk, int64_t Hq, int64_t Hkv, bool causal, int64_t B) {
          return shape_plan(D, B, Sq, Sk, Hq, Hkv, causal, AttnMask::Plain).bwd.one_block;
        }, "whether flash_bwd runs as the one-block short-sequence kernel (which can also emit the packed bias gradient)");
  m.def("flash_dropout_fused", [](int64_t D, int64_t Sq, int64_t Sk, int64_t Hq, int64_t Hkv, bool causal, int64_t B) {
          return shape_plan(D, B, Sq, Sk, Hq, Hkv, causal, AttnMask::Drop).ok;
        }, "whether flash_fwd / flash_bwd take dropout on the probabilities for this shape");
  m.def("flash_dkv_splits", [](int64_t B, int64_t Sq, int64_t Sk, int64_t Hkv, bool causal) {
          return shape_plan(128, B, Sq, Sk, Hkv, Hkv, causal, AttnMask::Plain).bwd.dkv_split;
        }, "chunks per key block of the dK/dV kernel (above 1: fp32 partials and a reduce pass)");
}

}  // namespace k8s_amd::binding
