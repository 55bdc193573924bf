// The rule a ReLU's backward applies in the gradient-only backward of the folded path (include/scouter_hip.h SCOUTER_RULE_*),
// defined ONCE for the four kernels that apply a ReLU mask there (relu_bwd of bn_elem.hip; sa_gate_bwd, sa_apply_relu_bwd and
// maxpool_relu_bwd of fold_bwd.hip).  g is the gradient arriving at the ReLU's output, y that output:
//   0 gradient    y > 0 ? g : +0                 the derivative
//   1 guided      (y > 0 && g > 0) ? g : +0      guided backpropagation (Springenberg et al. 2015)
//   2 deconvnet   g > 0 ? g : +0                 the deconvnet rule (Zeiler & Fergus 2014): y is not looked at
// Plain fp32 comparisons: a NaN or a -0 in g gives +0 under rules 1 and 2.  The rule is a compile-time argument; rule 0 is the
// expression the kernels had before there was a rule.
#pragma once
#include <type_traits>

#include "common.h"

constexpr int RULE_GRADIENT = 0, RULE_GUIDED = 1, RULE_DECONVNET = 2;

template <int RULE>
__device__ __forceinline__ float relu_rule(float g, float y) {
    if constexpr (RULE == RULE_GRADIENT) return y > 0.f ? g : 0.f;
    else if constexpr (RULE == RULE_GUIDED) return (y > 0.f && g > 0.f) ? g : 0.f;
    else return g > 0.f ? g : 0.f;
}

// whether the rule reads the activation at all: the deconvnet instantiations issue no load of it
template <int RULE>
constexpr bool rule_reads_activation = RULE != RULE_DECONVNET;

#define SC_REQUIRE_RULE(rule, what) \
    SC_REQUIRE((rule) >= RULE_GRADIENT && (rule) <= RULE_DECONVNET, what ": rule %d (0 gradient, 1 guided, 2 deconvnet)", (int)(rule))

// runs `launch(std::integral_constant<int, RULE>)` for the checked run-time rule
template <typename Launch>
static inline void rule_dispatch(int rule, Launch launch) {
    if (rule == RULE_GUIDED) launch(std::integral_constant<int, RULE_GUIDED>());
    else if (rule == RULE_DECONVNET) launch(std::integral_constant<int, RULE_DECONVNET>());
    else launch(std::integral_constant<int, RULE_GRADIENT>());
}
