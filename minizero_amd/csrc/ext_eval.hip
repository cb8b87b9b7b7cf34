// gfx950 kernels of the external evaluator's hand-over (ext_eval.h), built like every other unit (-ffp-contract=off).  Plain loads and vector stores, no
// atomics, no workgroup waits for another; every index is bounded by the shape the unit was initialised with.
#include "ext_eval.h"
#include "net_body.h"

namespace mz {

namespace {

// the value 1 in the caller's feature format (0 is all bits clear in all three)
template <class T> struct ExtOne;
template <> struct ExtOne<float> { static constexpr float v = 1.0f; };
struct ExtHalf { uint16_t bits; };  // f16 as its bits: 1.0 = 0x3C00
struct ExtBf16 { uint16_t bits; };  // bf16 as its bits: 1.0 = 0x3F80
template <> struct ExtOne<ExtHalf> { static constexpr uint16_t v = 0x3C00; };
template <> struct ExtOne<ExtBf16> { static constexpr uint16_t v = 0x3F80; };
template <class T> struct ExtRaw { using type = uint16_t; };
template <> struct ExtRaw<float> { using type = float; };

// exact widening of the caller's output formats
__device__ __forceinline__ float extWiden(float x) { return x; }
__device__ __forceinline__ float extWiden(ExtHalf x) { return static_cast<float>(__builtin_bit_cast(_Float16, x.bits)); }
__device__ __forceinline__ float extWiden(ExtBf16 x) { return __builtin_bit_cast(float, static_cast<uint32_t>(x.bits) << 16); }

// element e of the output [games][C][P], read from the bit planes [games][C][W32]: bit p & 31 of word p >> 5 of plane (g, c).  The planes of a game are
// contiguous on both sides, so (g, c) is one index: plane = e / P.
template <class T>
__device__ __forceinline__ typename ExtRaw<T>::type extPlaneBit(const uint32_t* __restrict__ bits, int P, int W32, unsigned e)
{
    const unsigned plane = e / unsigned(P), p = e - plane * unsigned(P);
    const uint32_t w = bits[size_t(plane) * W32 + (p >> 5)];
    return ((w >> (p & 31)) & 1u) ? ExtOne<T>::v : typename ExtRaw<T>::type(0);
}

// Export: thread t writes elements [VEC * t, VEC * t + VEC) of the flat output as ONE store of VEC elements (VEC = 4: 16 bytes of f32, 8 bytes of f16 / bf16;
// consecutive lanes write consecutive vectors).  The output is dense — planes are not padded, the last word of a plane is partial for every board but 8x8 —
// so a vector may straddle two planes or two games: every element finds its own word.  The words are read through the cache (32 elements share one).
// VEC = 1: a caller's tensor that is not aligned for the vector.
template <class T, int VEC>
__global__ void __launch_bounds__(256) ext_export_kernel(const uint32_t* __restrict__ bits, typename ExtRaw<T>::type* __restrict__ out, int P, int W32, unsigned total)
{
    const unsigned e0 = (blockIdx.x * 256u + threadIdx.x) * unsigned(VEC);
    if (e0 >= total) { return; }
    if constexpr (VEC > 1) {
        typedef typename ExtRaw<T>::type RV __attribute__((ext_vector_type(VEC)));
        if (e0 + VEC <= total) {
            RV v;
#pragma unroll
            for (int k = 0; k < VEC; ++k) { v[k] = extPlaneBit<T>(bits, P, W32, e0 + k); }
            *reinterpret_cast<RV*>(out + e0) = v;
            return;
        }
    }
    for (unsigned e = e0; e < total && e < e0 + VEC; ++e) { out[e] = extPlaneBit<T>(bits, P, W32, e); }
}

// Import: one wave per game.  Logits and value are widened and stored; the policy is the caller's, widened, or — policy == nullptr — the heads' softmax of
// the f32 logits, operation for operation (net_body.h headsBody, the wave-0 tail): the maximum, mz_expf(l - m), the index-order sum, the division.
// `lg` = A floats of LDS.
template <class T>
__global__ void __launch_bounds__(64) ext_import_kernel(const T* __restrict__ policy, const T* __restrict__ logits, const T* __restrict__ value,
                                                        float* __restrict__ d_policy, float* __restrict__ d_logit, float* __restrict__ d_value, int A)
{
    extern __shared__ float lg[];
    const int g = blockIdx.x, lane = threadIdx.x;
    const size_t off = size_t(g) * A;
    if (lane == 0) { d_value[g] = extWiden(value[g]); }
    for (int a = lane; a < A; a += 64) {
        const float l = extWiden(logits[off + a]);
        d_logit[off + a] = l;
        lg[a] = l;
    }
    if (policy) {
        for (int a = lane; a < A; a += 64) { d_policy[off + a] = extWiden(policy[off + a]); }
        return;
    }
    float m = -3.4e38f;
    for (int a = lane; a < A; a += 64) { m = lg[a] > m ? lg[a] : m; }
    for (int o = 32; o > 0; o >>= 1) { float m2 = __shfl_xor(m, o); m = m2 > m ? m2 : m; }
    for (int a = lane; a < A; a += 64) { lg[a] = mz_expf(lg[a] - m); }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const float s = orderedSumWave(lg, A, lane);
    for (int a = lane; a < A; a += 64) { d_policy[off + a] = lg[a] / s; }
}

constexpr int kExtMaxActions = 8192; // the import's LDS vector: 32 KB

const char* dtypeName(int t) { return t == MZ_F32 ? "f32" : t == MZ_F16 ? "f16" : "bf16"; }
size_t dtypeBytes(int t) { return t == MZ_F32 ? 4 : 2; }

} // namespace

class ExtEvalImpl final : public ExtEval {
public:
    int init(int device, hipStream_t stream, const ExtEvalShape& shape, const mz_evaluator& ev) override;
    int exportAsync(const uint32_t* feat_bits) override;
    int importAsync(float* d_policy, float* d_logit, float* d_value) override;
    const mz_evaluator& evaluator() const override { return ev_; }

private:
    template <class T> int exportT(const uint32_t* feat_bits);
    template <class T> int importT(float* d_policy, float* d_logit, float* d_value);
    ExtEvalShape s_{};
    mz_evaluator ev_{};
    hipStream_t stream_ = nullptr;
    int vec_ = 1;
    unsigned total_ = 0;
    DevBuf<float> own_feat_, own_out_; // library-owned buffers (ev.features == NULL)
};

ExtEval* createExtEval() { return new ExtEvalImpl(); }

int ExtEvalImpl::init(int device, hipStream_t stream, const ExtEvalShape& shape, const mz_evaluator& ev)
{
    s_ = shape;
    ev_ = ev;
    stream_ = stream;
    if (shape.games < 1 || shape.C < 1 || shape.P < 1 || shape.W32 != (shape.P + 31) / 32 || shape.A < 1 || shape.A > kExtMaxActions) {
        setError("external evaluator: unsupported shape (%d games, %d planes of %d points, %d actions)", shape.games, shape.C, shape.P, shape.A);
        return MZ_ERR_ARG;
    }
    const unsigned long long total = 1ull * shape.games * shape.C * shape.P;
    if (total >= (1ull << 31)) { setError("external evaluator: %llu feature elements per cycle do not fit the export's 32-bit index", total); return MZ_ERR_ARG; }
    total_ = static_cast<unsigned>(total);
    MZ_HIP(hipSetDevice(device));
    const size_t GA = size_t(shape.games) * shape.A;
    if (!ev.features) {
        if (ev.policy || ev.logits || ev.value) { setError("external evaluator: features is NULL (library-owned buffers) but an output pointer is given"); return MZ_ERR_ARG; }
        if (ev.feature_dtype != MZ_F32 || ev.output_dtype != MZ_F32) { setError("external evaluator: library-owned buffers are f32 (feature_dtype %d, output_dtype %d given)", ev.feature_dtype, ev.output_dtype); return MZ_ERR_ARG; }
        if (!own_feat_.alloc(total_) || !own_out_.alloc(2 * GA + shape.games)) { setError("external evaluator: allocation of the hand-over buffers failed"); return MZ_ERR_DEVICE; }
        MZ_HIP(hipMemset(own_out_.p, 0, own_out_.n * sizeof(float)));
        ev_.features = own_feat_.p;
        ev_.policy = own_out_.p;
        ev_.logits = own_out_.p + GA;
        ev_.value = own_out_.p + 2 * GA;
    } else if (!ev.logits || !ev.value) {
        setError("external evaluator: logits and value must be given with features (only policy may be NULL)");
        return MZ_ERR_ARG;
    }
    for (int t : {ev.feature_dtype, ev.output_dtype}) {
        if (t != MZ_F32 && t != MZ_F16 && t != MZ_BF16) { setError("external evaluator: dtype %d unknown (MZ_F32, MZ_F16, MZ_BF16)", t); return MZ_ERR_ARG; }
    }
    // every pointer aligned for its element; the features for the 4-element vector where they can be
    const size_t fb = dtypeBytes(ev_.feature_dtype), ob = dtypeBytes(ev_.output_dtype);
    if (reinterpret_cast<uintptr_t>(ev_.features) % fb) { setError("external evaluator: features pointer not aligned for %s", dtypeName(ev_.feature_dtype)); return MZ_ERR_ARG; }
    for (const void* p : {ev_.policy, ev_.logits, ev_.value}) {
        if (reinterpret_cast<uintptr_t>(p) % ob) { setError("external evaluator: an output pointer is not aligned for %s", dtypeName(ev_.output_dtype)); return MZ_ERR_ARG; }
    }
    vec_ = reinterpret_cast<uintptr_t>(ev_.features) % (4 * fb) == 0 ? 4 : 1;
    return MZ_OK;
}

template <class T>
int ExtEvalImpl::exportT(const uint32_t* feat_bits)
{
    using R = typename ExtRaw<T>::type;
    const unsigned threads = (total_ + vec_ - 1) / vec_, blocks = (threads + 255) / 256;
    if (vec_ == 4) { hipLaunchKernelGGL((ext_export_kernel<T, 4>), dim3(blocks), dim3(256), 0, stream_, feat_bits, static_cast<R*>(ev_.features), s_.P, s_.W32, total_); }
    else { hipLaunchKernelGGL((ext_export_kernel<T, 1>), dim3(blocks), dim3(256), 0, stream_, feat_bits, static_cast<R*>(ev_.features), s_.P, s_.W32, total_); }
    MZ_HIP(hipGetLastError());
    return MZ_OK;
}

int ExtEvalImpl::exportAsync(const uint32_t* feat_bits)
{
    switch (ev_.feature_dtype) {
    case MZ_F32: return exportT<float>(feat_bits);
    case MZ_F16: return exportT<ExtHalf>(feat_bits);
    default: return exportT<ExtBf16>(feat_bits);
    }
}

template <class T>
int ExtEvalImpl::importT(float* d_policy, float* d_logit, float* d_value)
{
    hipLaunchKernelGGL(ext_import_kernel<T>, dim3(s_.games), dim3(64), size_t(s_.A) * sizeof(float), stream_, static_cast<const T*>(ev_.policy),
                       static_cast<const T*>(ev_.logits), static_cast<const T*>(ev_.value), d_policy, d_logit, d_value, s_.A);
    MZ_HIP(hipGetLastError());
    return MZ_OK;
}

int ExtEvalImpl::importAsync(float* d_policy, float* d_logit, float* d_value)
{
    switch (ev_.output_dtype) {
    case MZ_F32: return importT<float>(d_policy, d_logit, d_value);
    case MZ_F16: return importT<ExtHalf>(d_policy, d_logit, d_value);
    default: return importT<ExtBf16>(d_policy, d_logit, d_value);
    }
}

} // namespace mz
