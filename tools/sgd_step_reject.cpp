// Host-only check of skdist_sgd_step's combination checks: every SgdStep
// below carries null device pointers and must come back as
// hipErrorInvalidValue before anything is launched, so this runs without a
// GPU and under a host sanitizer:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 \
//       -Xarch_host -fsanitize=address,undefined \
//       -Iskdist_amd/ops/csrc skdist_amd/ops/csrc/sgd_kernels.hip \
//       tools/sgd_step_reject.cpp -o /tmp/sgd_step_reject
//   /tmp/sgd_step_reject
#include <cstdio>

#include "sgd_api.h"

int main() {
    int word = 0;  // stands for a non-null table; never dereferenced
    struct Case { const char* what; SgdStep s; } cases[8];
    int n = 0;
    auto add = [&](const char* what) -> SgdStep& {
        cases[n].what = what;
        cases[n].s.m = 128;
        cases[n].s.ncols_pad = 128;
        return cases[n++].s;
    };
    { SgdStep& s = add("softmax, group_k 1"); s.loss_id = 3; s.group_k = 1; }
    { SgdStep& s = add("softmax, group_k 129"); s.loss_id = 3;
      s.group_k = 129; }
    { SgdStep& s = add("log loss, group_k 4"); s.group_k = 4; }
    { SgdStep& s = add("Tbits with softmax"); s.loss_id = 3; s.group_k = 4;
      s.Tbits = &word; }
    { SgdStep& s = add("Mbits without Tbits"); s.Mbits = &word; }
    { SgdStep& s = add("col_l1 alone"); s.col_l1 = &word; }
    { SgdStep& s = add("cpos and cneg without col_l1"); s.cpos = &word;
      s.cneg = &word; }
    { SgdStep& s = add("Tbits, col_l1 without cneg"); s.Tbits = &word;
      s.col_l1 = &word; s.cpos = &word; }
    int bad = 0;
    for (int i = 0; i < n; ++i) {
        const hipError_t err = skdist_sgd_step(cases[i].s, nullptr);
        const bool ok = err == hipErrorInvalidValue;
        std::printf("%-32s %s\n", cases[i].what,
                    ok ? "rejected" : hipGetErrorName(err));
        bad += !ok;
    }
    return bad != 0;
}
