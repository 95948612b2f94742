// Host (OpenMP) probabilistic kill / divide selection (World.kill_divide_prob on CPU worlds, and the
// oracle of the device kernels): the same per-cell decision as csrc/hip prob_masks_kernel, from the
// shared header.
#include <omp.h>

#include <stdexcept>
#include <utility>

#include "host_common.h"
#include "ms_select.h"

namespace ms_host {

using iarr = py::array_t<int32_t, py::array::c_style>;
using farr = py::array_t<float, py::array::c_style>;
using barr = py::array_t<uint8_t, py::array::c_style>;

// (kill, divide) uint8 masks over the n cells of mols (n, m) with genome lengths genome_lens (n).
// A term with enable false ignores its k / n. Nothing is paid here.
std::pair<barr, barr> prob_masks(farr mols, int mol, iarr genome_lens, bool kill_on, float kill_k, int kill_n,
                                 bool divide_on, float divide_k, int divide_n, bool genome_on, float genome_k,
                                 int genome_n, float kill_fraction, uint64_t seed, uint64_t call) {
  if (mols.ndim() != 2 || genome_lens.ndim() != 1 || genome_lens.shape(0) != mols.shape(0))
    throw std::invalid_argument("prob_masks: mols (n, m) and genome_lens (n)");
  const int64_t n = mols.shape(0), m = mols.shape(1);
  if (mol < 0 || mol >= m) throw std::invalid_argument("prob_masks: molecule index out of range");
  ms::SelectRule r{};
  r.mol = mol;
  r.kill_k = kill_k, r.divide_k = divide_k, r.genome_k = genome_k;
  r.kill_n = kill_n, r.divide_n = divide_n, r.genome_n = genome_n;
  r.enable = (kill_on ? ms::kSelKill : 0u) | (divide_on ? ms::kSelDivide : 0u) | (genome_on ? ms::kSelGenome : 0u);
  r.cost = 0.0f;
  r.kill_fraction = kill_fraction;
  barr kill({(py::ssize_t)n}), divide({(py::ssize_t)n});
  const float* x = mols.data();
  const int32_t* g = genome_lens.data();
  uint8_t* ko = kill.mutable_data();
  uint8_t* dv = divide.mutable_data();
  {
    py::gil_scoped_release nogil;
#pragma omp parallel for schedule(static) if (n > 4096)
    for (int64_t i = 0; i < n; ++i) {
      float u[4];
      ms::selection_uniforms(seed, call, (uint32_t)i, u);
      const int dec = ms::select_decide(r, x[i * m + mol], (float)g[i], u);
      ko[i] = dec & 1;
      dv[i] = (dec >> 1) & 1;
    }
  }
  return {kill, divide};
}

// The four uniforms of every cell 0..n-1 in the call (seed, call), float32 (n, 4)
farr selection_uniforms(int64_t n, uint64_t seed, uint64_t call, uint32_t first) {
  if (n < 0) throw std::invalid_argument("selection_uniforms: negative count");
  farr out({(py::ssize_t)n, (py::ssize_t)4});
  float* o = out.mutable_data();
  for (int64_t i = 0; i < n; ++i) ms::selection_uniforms(seed, call, first + (uint32_t)i, o + 4 * i);
  return out;
}

void bind_select(py::module_& m) {
  m.def("prob_masks", &prob_masks, py::arg("mols"), py::arg("mol"), py::arg("genome_lens"), py::arg("kill_on"),
        py::arg("kill_k"), py::arg("kill_n"), py::arg("divide_on"), py::arg("divide_k"), py::arg("divide_n"),
        py::arg("genome_on"), py::arg("genome_k"), py::arg("genome_n"), py::arg("kill_fraction"), py::arg("seed"),
        py::arg("call"), "Hill-curve kill / divide masks of kill_divide_prob (uint8 n each; no payment)");
  m.def("selection_uniforms", &selection_uniforms, py::arg("n"), py::arg("seed"), py::arg("call"),
        py::arg("first") = 0u, "the four selection uniforms of cells first..first+n-1, float32 (n, 4)");
}

}  // namespace ms_host
