// The one place where a Python tensor becomes a raw pointer for a kernel.
//
// The kernels dereference what they are given with no bounds checks, so an op builds one TensorArgs
// from its name and an anchor tensor and takes every pointer from it.  An accessor hands the pointer
// out only after it has checked that the tensor is defined, on the op's device, of the element type
// asked for, and large enough under one of two extent rules:
//   dense    at_least(n) / exactly(n): contiguous, numel() >= n or == n
//   strided  spans(n): an operand addressed through an explicit leading dimension; the op states
//            the elements it touches, (rows - 1) * ld + cols, the view must span that many
//            (1 + sum (size_i - 1) * stride_i) with a unit innermost stride.  A column slice of a
//            wider buffer passes; nothing past the view is ever read.
// Nothing is formatted unless a check fails.
#pragma once
#include <ATen/ATen.h>
#include <ATen/hip/HIPContext.h>
#include <c10/core/DeviceGuard.h>

#include "../kernels/common.h"

namespace dtfe {

inline bool has(const c10::optional<at::Tensor>& t) { return t.has_value() && t->defined(); }

struct Extent { int64_t n; bool exact, strided; };
inline Extent at_least(int64_t n) { return {n, false, false}; }
inline Extent exactly(int64_t n) { return {n, true, false}; }
inline Extent spans(int64_t n) { return {n, false, true}; }

// element type of a pointer <-> the scalar types it may point into
template <typename T> struct Elem;
#define DTFE_ELEM(T, COND, NAME)                                      \
  template <> struct Elem<T> {                                        \
    static bool ok(const at::Tensor& t) { return COND; }              \
    static constexpr const char* name = NAME;                         \
  }
DTFE_ELEM(float, t.scalar_type() == at::kFloat, "float32");
DTFE_ELEM(bf16, t.scalar_type() == at::kBFloat16, "bfloat16");
DTFE_ELEM(uint8_t, t.scalar_type() == at::kByte, "uint8");
DTFE_ELEM(int32_t, t.scalar_type() == at::kInt, "int32");
DTFE_ELEM(int64_t, t.scalar_type() == at::kLong, "int64");
DTFE_ELEM(uint64_t, t.scalar_type() == at::kLong, "int64");
DTFE_ELEM(uint32_t, t.element_size() == 4, "4-byte");  // counters and tickets: any 32-bit word
#undef DTFE_ELEM

// dtype codes of the two-dtype arguments (GatherArgs::src_dtype and friends); an allowed set is a mask of 1 << code
enum DataCode : int { DATA_U8 = 0, DATA_F32 = 1, DATA_BF16 = 2 };
constexpr unsigned F32_OR_BF16 = 1u << DATA_F32 | 1u << DATA_BF16, U8_OR_F32 = 1u << DATA_U8 | 1u << DATA_F32,
                   ANY_DATA = F32_OR_BF16 | 1u << DATA_U8;
struct AnyPtr { void* p; int code; bool f32() const { return code == DATA_F32; } };

class TensorArgs {
 public:
  // anchor: a GPU tensor; its device is the op's device and is current until this object goes
  TensorArgs(const char* op, const at::Tensor& anchor, const char* anchor_name)
      : op_(op), dev_(gpu_of(op, anchor, anchor_name)), guard_(dev_) {}

  hipStream_t stream() const { return at::hip::getCurrentHIPStream(dev_.index()).stream(); }
  c10::Device device() const { return dev_; }

  template <typename T> const T* in(const at::Tensor& t, const char* name, Extent e) const {
    if (C10_UNLIKELY(!(usable(t, e) && Elem<T>::ok(t)))) refuse(t, name, Elem<T>::name, e);
    return static_cast<const T*>(t.data_ptr());
  }
  template <typename T> T* out(const at::Tensor& t, const char* name, Extent e) const {
    return const_cast<T*>(in<T>(t, name, e));
  }
  // an absent optional tensor: nullptr
  template <typename T> const T* in(const c10::optional<at::Tensor>& t, const char* name, Extent e) const {
    return has(t) ? in<T>(*t, name, e) : nullptr;
  }
  template <typename T> T* out(const c10::optional<at::Tensor>& t, const char* name, Extent e) const {
    return has(t) ? out<T>(*t, name, e) : nullptr;
  }
  // an argument of one of several dtypes (allowed: a mask of 1 << DataCode)
  AnyPtr any(const at::Tensor& t, const char* name, unsigned allowed, Extent e) const {
    const int code = !t.defined() ? -1 : t.scalar_type() == at::kByte ? DATA_U8 : t.scalar_type() == at::kFloat ? DATA_F32
                   : t.scalar_type() == at::kBFloat16 ? DATA_BF16 : -1;
    if (C10_UNLIKELY(code < 0 || !(allowed >> code & 1) || !usable(t, e)))
      refuse(t, name, allowed == F32_OR_BF16 ? "float32 or bfloat16" : allowed == U8_OR_F32 ? "uint8 or float32"
                                                                                             : "uint8, float32 or bfloat16", e);
    return {t.data_ptr(), code};
  }
  AnyPtr any(const c10::optional<at::Tensor>& t, const char* name, unsigned allowed, Extent e) const {
    return has(t) ? any(*t, name, allowed, e) : AnyPtr{nullptr, -1};
  }

  // the step's accumulators that a launch clears: at most 4 ranges, each contiguous whole 32-bit words
  template <typename Z> void zero_ranges(const Z& zero, uint32_t* (&zptr)[4], long (&zlen)[4], int& nz) const {
    TORCH_CHECK(zero.size() <= 4, op_, ": at most 4 zero ranges");
    nz = 0;
    for (const at::Tensor& z : zero) {
      TORCH_CHECK(z.defined() && z.device() == dev_ && z.is_contiguous() && (z.numel() * z.element_size()) % 4 == 0, op_,
                  ": zero ranges must be contiguous whole 32-bit words on ", dev_);
      zptr[nz] = static_cast<uint32_t*>(z.data_ptr());
      zlen[nz++] = (long)(z.numel() * z.element_size() / 4);
    }
  }

 private:
  static int64_t span(const at::Tensor& t) {
    if (t.numel() == 0) return 0;
    int64_t s = 1;
    for (int64_t i = 0; i < t.dim(); ++i) s += (t.size(i) - 1) * t.stride(i);
    return s;
  }
  bool usable(const at::Tensor& t, Extent e) const {
    if (!t.defined() || t.device() != dev_) return false;
    if (e.strided) return (t.dim() == 0 || t.size(-1) == 1 || t.stride(-1) == 1) && span(t) >= e.n;
    return t.is_contiguous() && (e.exact ? t.numel() == e.n : t.numel() >= e.n);
  }
  [[noreturn]] void refuse(const at::Tensor& t, const char* name, const char* dtype, Extent e) const {
    TORCH_CHECK(t.defined(), op_, ": ", name, " is required (", dtype, " on ", dev_, ")");
    TORCH_CHECK(false, op_, ": ", name, " must be ", dtype, " on ", dev_,
                e.strided ? ", rows of unit stride spanning at least " : e.exact ? ", contiguous with exactly "
                                                                                 : ", contiguous with at least ",
                e.n, " elements; got ", t.scalar_type(), " on ", t.device(), ", sizes ", t.sizes(), ", strides ",
                t.strides(), " (numel ", t.numel(), ", span ", span(t), ")");
  }
  static c10::Device gpu_of(const char* op, const at::Tensor& t, const char* name) {
    TORCH_CHECK(t.defined() && t.is_cuda(), op, ": ", name, " must be on the GPU (HIP) device");
    return t.device();
  }

  const char* op_;
  c10::Device dev_;
  c10::DeviceGuard guard_;
};

}  // namespace dtfe
