// External evaluator (mz_worker_create_external, include/mzgpu.h): the hand-over between the worker's resident lock-step cycle and the caller's network.
// The cycle keeps its four steps on the lane's stream — leafAsync, the network, candAsync, expandBackupAsync — and the network step becomes
//   ext_export_kernel   the leaf planes from their bit-packed form (GoDevView::feat, [games][C][W32] words) into the caller's tensor [games][C][P]
//   (the worker waits for the stream and calls the caller's forward(), which returns with its outputs complete)
//   ext_import_kernel   the caller's policy / logits / value into the lane's f32 d_policy / d_logit / d_value; without a policy it is the softmax of the
//                       logits in the heads' own arithmetic (net_body.h headsBody), so logits of the library's own heads give the heads' policy bit for bit
// Nothing is computed that the heads do not compute: 0 and 1 are exact in f32, f16 and bf16, and widening f16 / bf16 to f32 is exact.
#pragma once
#include "common.h"

namespace mz {

// the shapes of the hand-over: what the device rules write and what the caller's tensors hold
struct ExtEvalShape {
    int games, C, P, W32, A;
};

// The device half behind an interface, as think.h and tree_read.h do it: the worker reaches it through createExtEval(), which ext_eval.hip defines; where
// that unit is not linked (the host-only test programs) the symbol is null and mz_worker_create_external says so.
class ExtEval {
public:
    virtual ~ExtEval() = default;
    // ev.features == NULL: the four buffers are allocated here (f32 features, f32 outputs, a policy included)
    virtual int init(int device, hipStream_t stream, const ExtEvalShape& shape, const mz_evaluator& ev) = 0;
    virtual int exportAsync(const uint32_t* feat_bits) = 0;
    virtual int importAsync(float* d_policy, float* d_logit, float* d_value) = 0;
    virtual const mz_evaluator& evaluator() const = 0; // the pointers in use
};
ExtEval* createExtEval() __attribute__((weak));

} // namespace mz
