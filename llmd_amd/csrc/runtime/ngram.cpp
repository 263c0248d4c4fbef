// N-gram (prompt-lookup) draft proposer for speculative decoding: one index per
// request over its prompt + output tokens. For every n in [min_n, max_n] a map
// from the hash of an n-gram to the position right after its most recent
// occurrence that already has a successor; `propose(k)` takes the longest n
// whose suffix n-gram occurred earlier and returns up to k tokens that followed.
// `append` costs O(new tokens * (max_n - min_n + 1) * max_n), `propose` O(max_n^2).
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <unordered_map>
#include <vector>

#include "hashing.h"

namespace py = pybind11;

namespace {

class NgramIndex {
 public:
  NgramIndex(int min_n, int max_n) : min_n_(min_n), max_n_(max_n) {
    if (min_n < 1 || max_n < min_n) throw std::invalid_argument("NgramIndex: need 1 <= min_n <= max_n");
  }

  void append(const std::vector<int32_t>& toks) {
    for (int32_t t : toks) {
      // the n-grams ending at the previous token gain a successor (this one): register them
      const int64_t i = (int64_t)toks_.size();  // index of t
      for (int n = min_n_; n <= max_n_ && n <= i; ++n) map_[key(i - n, n)] = (int32_t)i;
      toks_.push_back(t);
    }
  }

  std::vector<int32_t> propose(int k) const {
    const int64_t len = (int64_t)toks_.size();
    if (k <= 0) return {};
    for (int n = (int)std::min<int64_t>(max_n_, len); n >= min_n_; --n) {
      auto it = map_.find(key(len - n, n));
      if (it == map_.end()) continue;
      const int64_t pos = it->second;  // position after the earlier occurrence
      bool same = true;                // a hash hit is only a candidate
      for (int j = 0; j < n && same; ++j) same = toks_[pos - n + j] == toks_[len - n + j];
      if (!same) continue;
      const int64_t end = std::min<int64_t>(len, pos + k);
      return std::vector<int32_t>(toks_.begin() + pos, toks_.begin() + end);
    }
    return {};
  }

  int64_t size() const { return (int64_t)toks_.size(); }

 private:
  uint64_t key(int64_t first, int n) const {
    return llmd_rt::hash_block(llmd_rt::kRootHash, (uint64_t)n, toks_.data() + first, (size_t)n);
  }

  int min_n_, max_n_;
  std::vector<int32_t> toks_;
  std::unordered_map<uint64_t, int32_t> map_;
};

}  // namespace

void register_ngram(py::module_& m) {
  py::class_<NgramIndex>(m, "NgramIndex")
      .def(py::init<int, int>(), py::arg("min_n"), py::arg("max_n"))
      .def("append", &NgramIndex::append, py::arg("tokens"))
      .def("propose", &NgramIndex::propose, py::arg("k"))
      .def("__len__", &NgramIndex::size);
}
