// fwd_choice_sweep.cpp — the sweep of tests/test_fwd_choice.py straight against csrc/fa_fwd_f16_choice.h and the
// band's conditions, as a host program of its own for the sanitizers (the predicates multiply 64-bit extents).
// CPU only; it launches nothing.  Build and run from the repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -Iinclude tools/fwd_choice_sweep.cpp \
//         tf_flash_attention_amd/csrc/fa_fwd_f16_band.hip -o tools/fwd_choice_sweep && tools/fwd_choice_sweep
#include <stdio.h>

#include <set>
#include <string>

#include "../tf_flash_attention_amd/csrc/fa_device.h"
#include "../tf_flash_attention_amd/csrc/fa_fwd_f16_choice.h"

namespace fa {  // what fa_fwd_f16_band.hip takes from fa_api.hip: an MI355X without a partition
hipError_t set_smem_once(const void*, int) { return hipSuccess; }
int device_cus() { return 256; }
int device_xcds() { return 8; }
}  // namespace fa

int main() {
  const int channels[] = {16, 32, 33, 64, 65, 128, 129, 256}, lengths[] = {1, 8, 72, 136, 264, 4096, 0x7fffffff};
  const int64_t batches[] = {1, 2, 1024, (1ll << 31) - 1, 1ll << 31, 1ll << 62, INT64_MAX};
  const uintptr_t offs[][3] = {{0, 0, 0}, {0, 8, 0}, {2, 0, 2}};
  const int variants[] = {-1, 146, 308, 408, 1814, 2000, 2200, 2301, 2402, 2600, 2701};
  std::set<std::string> product;
  long n = 0;
  for (int policy = 0; policy < 3; ++policy)
    for (int dims = 1; dims <= 2; ++dims)
      for (int ls = 0; ls < 2; ++ls)
        for (int nq : lengths)
          for (int nk : lengths) {
            fa::FwdArgs a = {};
            fa::Rule& r = a.rule;
            r.policy = policy, r.seq_dims = dims, r.ls = ls, r.ws = 64, r.sws = 64 << ls, r.look_ahead = r.sws;
            r.log2R0 = dims == 1 ? 30 : 15, r.R0 = 1 << r.log2R0, r.log2R1 = 15, r.R1 = 1 << 15;
            r.q = {nq, dims == 1 ? nq : 8, 1, 0, 1, 0};
            r.k = {nk, dims == 1 ? nk : 8, 1, 0, 1, 0};
            for (int d : channels)
              for (int vd : channels)
                for (auto& o : offs)
                  for (int64_t b : batches)
                    for (int v : variants) {
                      a.Q = (void*)((1 << 20) + o[0]), a.K = (void*)((1 << 20) + o[1]), a.V = (void*)((1 << 20) + o[2]);
                      a.b = b, a.d = d, a.v_d = vd;
                      const std::string name = fa::fwd_f16_choice_name(fa::fwd_f16_choice(a, 8, v));
                      if (v < 0) product.insert(name);
                      ++n;
                    }
          }
  for (const std::string& s : product) {
    printf("%s\n", s.c_str());
    if (s.find("pingpong128") != s.npos || (s.find("fast_kernel") != s.npos && s.find(", 0, ") != s.npos)) return 1;
  }
  printf("%ld choices, %zu product kernels, no sanitizer report\n", n, product.size());
  return 0;
}
