// The batched exchange overloads of include/helfem_gpu_arma.hpp, instantiated against the stand-in matrix class on both
// basis classes: tests/test_exchange_batch_cpu.py compiles this file (syntax only; the entries behind the overloads are
// tested on the device in tests/test_gpu_exchange_batch.py).
#include "../../include/helfem_gpu_arma.hpp"
#include "../../helfem_amd/csrc/host/linalg.h"

using helfem::Mat;
namespace hg = helfem::gpu;

std::vector<Mat> diatomic_exchange(const hg::diatomic::TwoDBasis<Mat> &basis, const std::vector<Mat> &P) { return basis.exchange(P); }
std::vector<Mat> atomic_exchange(const hg::atomic::TwoDBasis<Mat> &basis, const std::vector<Mat> &P) { return basis.exchange(P); }
std::vector<Mat> atomic_rs_exchange(const hg::atomic::TwoDBasis<Mat> &basis, const std::vector<Mat> &P) { return basis.rs_exchange(P); }
Mat single_still_binds(const hg::atomic::TwoDBasis<Mat> &basis, const Mat &P) { return basis.exchange(P); }
