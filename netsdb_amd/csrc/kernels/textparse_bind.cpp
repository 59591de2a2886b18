// PyTorch bindings of the delimited-text parser (textparse.hip). The binding sizes every allocation from
// textparse_plan.h and from the counts the kernels report; the launcher launches what the plan says.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "textparse_plan.h"

extern "C" {
int nsdb_textparse_plan(long long nbytes, int nfields, int delimiter, long long* fields);
int nsdb_textparse_index(const void* buf, long long n, long long alloc, int nfields, int delimiter, unsigned* counts,
                         unsigned long long* state, hipStream_t st);
int nsdb_textparse_decode(const void* buf, long long n, long long alloc, const unsigned char* kinds, void* const* outs,
                          int nfields, int delimiter, int trailing, long long rows, const unsigned* counts,
                          unsigned* starts, unsigned long long* state, unsigned long long* list, long long cap,
                          int write_rows, hipStream_t st);
}

namespace {

hipStream_t stream() { return c10::hip::getCurrentHIPStream().stream(); }

void rc_ok(int rc, const char* what) {
  TORCH_CHECK(rc == 0, what, " failed with code ", rc, " (", hipGetErrorString((hipError_t)(rc > 0 ? rc : 0)), ")");
}

const char* plan_refusal(int rc) {
  switch (rc) {
    case nsdb::TEXT_EMPTY: return "empty buffer";
    case nsdb::TEXT_TOO_LARGE: return "buffer of 2^31 bytes or more";
    case nsdb::TEXT_BAD_NFIELDS: return "fields per row outside 1..64";
    case nsdb::TEXT_BAD_DELIM: return "delimiter is not one byte, or is a line end";
    default: return "ok";
  }
}

pybind11::dict text_parse_plan(int64_t nbytes, int64_t nfields, int64_t delimiter) {
  long long f[8];
  nsdb_textparse_plan(nbytes, (int)std::clamp<int64_t>(nfields, -1, 1 << 20), (int)std::clamp<int64_t>(delimiter, -1, 256),
                      f);
  pybind11::dict d;
  const char* names[8] = {"rc", "tile", "tiles", "scan_step", "launches", "counts_bytes", "state_bytes",
                          "scratch_bytes"};
  for (int i = 0; i < 8; ++i) d[names[i]] = (int64_t)f[i];
  return d;
}

// One chunk of whole lines -> (host [rows, error code, bad row, flagged cells], one tensor per field of the file (an
// undefined one for a skipped field, [2, rows] int64 starts / ends for a string field), the flagged cells as
// [cells, 2] int64 (row << 8 | field, start << 32 | end) or an undefined tensor). payload bytes of buf are text; loads
// stay inside buf. Two host reads: the row count sizes the outputs, then the status words; a third launch and nothing
// more when cells were flagged. On an error code the columns are not to be used.
std::tuple<torch::Tensor, std::vector<torch::Tensor>, torch::Tensor> text_parse(torch::Tensor buf, int64_t payload,
                                                                                std::vector<int64_t> kinds,
                                                                                int64_t delimiter, bool trailing) {
  TORCH_CHECK(buf.is_cuda() && buf.scalar_type() == torch::kUInt8 && buf.dim() == 1 && buf.is_contiguous(),
              "text_parse: buf must be a contiguous 1-D uint8 GPU tensor");
  TORCH_CHECK_VALUE(payload <= buf.numel(), "text_parse: payload exceeds the buffer");
  const int nf = (int)std::min<size_t>(kinds.size(), 1 << 20);
  long long pf[8];
  const int prc = nsdb_textparse_plan(payload, nf, (int)std::clamp<int64_t>(delimiter, -1, 256), pf);
  TORCH_CHECK_VALUE(prc == nsdb::TEXT_OK, "text_parse: ", plan_refusal(prc));
  for (int64_t k : kinds) TORCH_CHECK_VALUE(k >= nsdb::TEXT_SKIP && k <= nsdb::TEXT_STR, "text_parse: no such field kind");
  if (reinterpret_cast<uintptr_t>(buf.data_ptr()) & 15) buf = buf.clone();   // 16-byte loads
  // no load passes the allocation; nor does one need more of it than the payload's last 16-byte block
  const int64_t alloc = std::min<int64_t>(buf.numel(), (payload + 15) & ~int64_t(15));
  auto i64o = buf.options().dtype(torch::kInt64);
  auto scratch = torch::empty({pf[7] / 8 + 1}, i64o);                        // state (4 u64) | counts
  auto* state = reinterpret_cast<unsigned long long*>(scratch.data_ptr<int64_t>());
  auto* counts = reinterpret_cast<unsigned*>(state + nsdb::kTextStateWords);
  rc_ok(nsdb_textparse_index(buf.data_ptr(), payload, alloc, nf, (int)delimiter, counts, state, stream()),
        "textparse_index");
  const int64_t rows = scratch[0].item<int64_t>();
  std::vector<torch::Tensor> cols(nf);
  std::vector<void*> outs(nf, nullptr);
  std::vector<unsigned char> kd(nf);
  for (int f = 0; f < nf; ++f) {
    kd[f] = (unsigned char)kinds[f];
    switch (kinds[f]) {
      case nsdb::TEXT_INT: cols[f] = torch::empty({rows}, i64o); break;
      case nsdb::TEXT_FLOAT: cols[f] = torch::empty({rows}, buf.options().dtype(torch::kFloat64)); break;
      case nsdb::TEXT_BOOL: cols[f] = torch::empty({rows}, buf.options().dtype(torch::kBool)); break;
      case nsdb::TEXT_DATE: cols[f] = torch::empty({rows}, buf.options().dtype(torch::kInt32)); break;
      case nsdb::TEXT_STR: cols[f] = torch::empty({2, rows}, i64o); break;
      default: break;
    }
    if (cols[f].defined()) outs[f] = cols[f].data_ptr();
  }
  auto starts = torch::empty({rows + 1}, buf.options().dtype(torch::kInt32));
  auto* sp = reinterpret_cast<unsigned*>(starts.data_ptr<int32_t>());
  rc_ok(nsdb_textparse_decode(buf.data_ptr(), payload, alloc, kd.data(), outs.data(), nf, (int)delimiter, trailing, rows,
                              counts, sp, state, nullptr, 0, 1, stream()),
        "textparse_decode");
  auto host = scratch.slice(0, 0, nsdb::kTextStateWords).cpu();
  auto h = host.accessor<int64_t, 1>();
  auto stats = torch::zeros({4}, torch::kInt64);
  auto s = stats.accessor<int64_t, 1>();
  s[0] = rows;
  s[3] = h[2];
  if (h[1] != -1) {                                                          // the lowest bad row and its code
    s[1] = h[1] & 0xFF;
    s[2] = (int64_t)((unsigned long long)h[1] >> 8);
    return {stats, cols, torch::Tensor()};
  }
  torch::Tensor list;
  if (h[2] > 0) {                                                            // the same walk again, listing the cells
    list = torch::empty({h[2], 2}, i64o);
    scratch.slice(0, 2, 3).zero_();
    rc_ok(nsdb_textparse_decode(buf.data_ptr(), payload, alloc, kd.data(), outs.data(), nf, (int)delimiter, trailing,
                                rows, counts, sp, state, reinterpret_cast<unsigned long long*>(list.data_ptr<int64_t>()),
                                h[2], 0, stream()),
          "textparse_decode (flagged cells)");
  }
  return {stats, cols, list};
}

}  // namespace

void register_textparse(pybind11::module& m) {
  m.def("text_parse_plan", &text_parse_plan, "plan of text_parse for a buffer of nbytes with nfields per row: rc, tile, "
        "tiles, scan_step, launches and the scratch bytes by buffer; launches nothing", pybind11::arg("nbytes"),
        pybind11::arg("nfields"), pybind11::arg("delimiter") = 124);
  m.def("text_parse", &text_parse, "delimited text -> (host [rows, error code, bad row, flagged cells], one tensor per "
        "field, flagged cells)", pybind11::arg("buf"), pybind11::arg("payload"), pybind11::arg("kinds"),
        pybind11::arg("delimiter") = 124, pybind11::arg("trailing") = true);
}
