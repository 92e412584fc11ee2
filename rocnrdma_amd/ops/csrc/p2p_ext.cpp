// SPDX-License-Identifier: MIT
// Torch bindings for the gfx950 payload kernels (p2p_kernels.hip).
// Thin: tensor checks + stream plumbing only; all device logic lives in
// the .hip TU.  Fails loudly — there is deliberately NO CPU fallback
// here, so a GPU test that silently skipped the native path is
// impossible (CPU references for tests live in rocnrdma_amd/utils).
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <c10/cuda/CUDAGuard.h>

#include "p2p_kernels.h"
#include "p2p_sgl.h"  // ROCP2P_SGL_SCRATCH_WORDS
#include "p2p_prot.h"  // ROCP2P_PROT_SCRATCH_WORDS

namespace {

const torch::Tensor& check_buf(const torch::Tensor& t, const char* who) {
  TORCH_CHECK(t.is_cuda(), who, ": tensor must be on GPU");
  TORCH_CHECK(t.is_contiguous(), who, ": tensor must be contiguous");
  return t;
}

// How every binding starts: check the tensor it works on, make that
// tensor's device current until the binding returns (allocations and
// the launch follow the tensor, not whatever device the caller left
// current), and pick up that device's current stream.
struct OnDeviceOf {
  c10::cuda::CUDAGuard guard;
  hipStream_t stream;
  OnDeviceOf(const torch::Tensor& t, const char* who)
      : guard(check_buf(t, who).device()),
        stream(at::cuda::getCurrentCUDAStream().stream()) {}
};

uint64_t nbytes_of(const torch::Tensor& t) {
  return (uint64_t)t.numel() * t.element_size();
}

#define HIP_OK(expr)                                              \
  do {                                                            \
    hipError_t _e = (expr);                                       \
    TORCH_CHECK(_e == hipSuccess, #expr, " failed: ",             \
                hipGetErrorString(_e));                           \
  } while (0)

void fill_(torch::Tensor buf, int64_t seed) {
  OnDeviceOf dev(buf, "fill_");
  HIP_OK(rocp2p_fill(buf.data_ptr(), nbytes_of(buf), (uint64_t)seed,
                     dev.stream));
}

int64_t verify(torch::Tensor buf, int64_t seed) {
  OnDeviceOf dev(buf, "verify");
  auto mis = torch::zeros({1}, torch::dtype(torch::kInt64).device(buf.device()));
  HIP_OK(rocp2p_verify(buf.data_ptr(), nbytes_of(buf), (uint64_t)seed,
                       (unsigned long long*)mis.data_ptr<int64_t>(),
                       dev.stream));
  return mis.item<int64_t>();
}

torch::Tensor crc32_pages(torch::Tensor buf) {
  OnDeviceOf dev(buf, "crc32_pages");
  uint64_t nbytes = nbytes_of(buf);
  TORCH_CHECK(nbytes % 4096 == 0, "crc32_pages: length must be 4 KiB pages");
  int64_t npages = (int64_t)(nbytes / 4096);
  auto out =
      torch::empty({npages}, torch::dtype(torch::kInt32).device(buf.device()));
  HIP_OK(rocp2p_crc32_pages(buf.data_ptr(), (uint64_t)npages,
                            (uint32_t*)out.data_ptr<int32_t>(),
                            dev.stream));
  return out;
}

void check_u64_dev(const torch::Tensor& t, const char* who) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
                  t.scalar_type() == torch::kInt64,
              who, ": descriptor tensor must be contiguous int64 on GPU");
}

void check_align16(const torch::Tensor& t, const char* who) {
  TORCH_CHECK((uintptr_t)t.data_ptr() % 16 == 0, who,
              ": base address must be 16-byte aligned");
}

torch::Tensor crc32_messages(torch::Tensor region, int64_t msg_bytes,
                             c10::optional<torch::Tensor> offs,
                             int64_t grid_cap) {
  OnDeviceOf dev(region, "crc32_messages");
  check_align16(region, "crc32_messages");
  TORCH_CHECK(msg_bytes > 0 && msg_bytes % 16 == 0,
              "crc32_messages: msg_bytes must be a non-zero multiple of 16");
  TORCH_CHECK(grid_cap >= 0 && grid_cap <= 0xffffffffLL,
              "crc32_messages: grid_cap out of range");
  uint64_t nbytes = nbytes_of(region);
  int64_t n;
  const uint64_t* d_offs = nullptr;
  if (offs.has_value()) {
    check_u64_dev(*offs, "crc32_messages");
    TORCH_CHECK(offs->device() == region.device(),
                "crc32_messages: offs must live on the region's device");
    n = offs->numel();
    d_offs = (const uint64_t*)offs->data_ptr<int64_t>();
  } else {
    TORCH_CHECK(nbytes % (uint64_t)msg_bytes == 0,
                "crc32_messages: region length must be a multiple of "
                "msg_bytes");
    n = (int64_t)(nbytes / (uint64_t)msg_bytes);
  }
  TORCH_CHECK(n < (1LL << 32), "crc32_messages: too many messages");
  auto out =
      torch::empty({n}, torch::dtype(torch::kInt32).device(region.device()));
  if (!n) return out;
  HIP_OK(rocp2p_crc32_msgs(region.data_ptr(), d_offs, (uint64_t)msg_bytes,
                           (uint32_t)n, (uint32_t*)out.data_ptr<int32_t>(),
                           (uint32_t)grid_cap, dev.stream));
  return out;
}

int64_t crc32(torch::Tensor buf, int64_t grid_cap) {
  OnDeviceOf dev(buf, "crc32");
  check_align16(buf, "crc32");
  TORCH_CHECK(grid_cap >= 0 && grid_cap <= 0xffffffffLL,
              "crc32: grid_cap out of range");
  uint64_t nbytes = nbytes_of(buf);
  auto out =
      torch::empty({1}, torch::dtype(torch::kInt32).device(buf.device()));
  HIP_OK(rocp2p_crc32_region(buf.data_ptr(), nbytes,
                             (uint32_t*)out.data_ptr<int32_t>(),
                             (uint32_t)grid_cap, dev.stream));
  return (int64_t)(uint32_t)out.item<int32_t>();
}

void gather_(torch::Tensor region, torch::Tensor dst_offs,
             torch::Tensor src_addrs, int64_t msg_bytes) {
  OnDeviceOf dev(region, "gather_");
  check_u64_dev(dst_offs, "gather_");
  check_u64_dev(src_addrs, "gather_");
  TORCH_CHECK(dst_offs.numel() == src_addrs.numel(), "gather_: n mismatch");
  HIP_OK(rocp2p_gather(region.data_ptr(),
                       (const uint64_t*)dst_offs.data_ptr<int64_t>(),
                       (const uint64_t*)src_addrs.data_ptr<int64_t>(),
                       (uint64_t)msg_bytes, (uint32_t)dst_offs.numel(),
                       dev.stream));
}

void scatter_(torch::Tensor region, torch::Tensor src_offs,
              torch::Tensor dst_addrs, int64_t msg_bytes) {
  OnDeviceOf dev(region, "scatter_");
  check_u64_dev(src_offs, "scatter_");
  check_u64_dev(dst_addrs, "scatter_");
  TORCH_CHECK(src_offs.numel() == dst_addrs.numel(), "scatter_: n mismatch");
  HIP_OK(rocp2p_scatter(region.data_ptr(),
                        (const uint64_t*)src_offs.data_ptr<int64_t>(),
                        (const uint64_t*)dst_addrs.data_ptr<int64_t>(),
                        (uint64_t)msg_bytes, (uint32_t)src_offs.numel(),
                        dev.stream));
}

// gather_/scatter_ with the inline ICRC: same checks and prologue, plus
// the digest tensor (int32[n] on the region's device, no sync).
template <typename Launch>
torch::Tensor msg_engine_crc(const char* who, Launch launch,
                             torch::Tensor region, torch::Tensor offs,
                             torch::Tensor addrs, int64_t msg_bytes,
                             int64_t grid_cap) {
  OnDeviceOf dev(region, who);
  check_u64_dev(offs, who);
  check_u64_dev(addrs, who);
  TORCH_CHECK(offs.numel() == addrs.numel(), who, ": n mismatch");
  TORCH_CHECK(grid_cap >= 0 && grid_cap <= 0xffffffffLL, who,
              ": grid_cap out of range");
  auto out = torch::empty({offs.numel()},
                          torch::dtype(torch::kInt32).device(region.device()));
  HIP_OK(launch(region.data_ptr(), (const uint64_t*)offs.data_ptr<int64_t>(),
                (const uint64_t*)addrs.data_ptr<int64_t>(),
                (uint64_t)msg_bytes, (uint32_t)offs.numel(),
                (uint32_t*)out.data_ptr<int32_t>(), (uint32_t)grid_cap,
                dev.stream));
  return out;
}

torch::Tensor gather_crc_(torch::Tensor region, torch::Tensor dst_offs,
                          torch::Tensor src_addrs, int64_t msg_bytes,
                          int64_t grid_cap) {
  return msg_engine_crc("gather_crc_", rocp2p_gather_crc, region, dst_offs,
                        src_addrs, msg_bytes, grid_cap);
}

torch::Tensor scatter_crc_(torch::Tensor region, torch::Tensor src_offs,
                           torch::Tensor dst_addrs, int64_t msg_bytes,
                           int64_t grid_cap) {
  return msg_engine_crc("scatter_crc_", rocp2p_scatter_crc, region, src_offs,
                        dst_addrs, msg_bytes, grid_cap);
}

// The per-message-length forms: same checks, plus the length tensor;
// the n + 1 words of scan scratch and the digests are torch tensors, so
// the caching allocator keeps them alive until the stream has used them.
struct VarLenArgs {
  int64_t n;
  torch::Tensor cstart;
  VarLenArgs(const char* who, const torch::Tensor& region,
             const torch::Tensor& offs, const torch::Tensor* addrs,
             const torch::Tensor& lens, int64_t max_msg_bytes,
             int64_t grid_cap) {
    check_align16(region, who);
    check_u64_dev(offs, who);
    if (addrs) check_u64_dev(*addrs, who);
    check_u64_dev(lens, who);
    n = offs.numel();
    TORCH_CHECK(lens.numel() == n && (!addrs || addrs->numel() == n), who,
                ": n mismatch");
    TORCH_CHECK(offs.device() == region.device() &&
                    lens.device() == region.device() &&
                    (!addrs || addrs->device() == region.device()),
                who, ": descriptors must live on the region's device");
    TORCH_CHECK(n < (1LL << 32), who, ": too many messages");
    TORCH_CHECK(max_msg_bytes >= 0, who, ": max_msg_bytes out of range");
    TORCH_CHECK(grid_cap >= 0 && grid_cap <= 0xffffffffLL, who,
                ": grid_cap out of range");
    cstart = torch::empty(
        {n + 1}, torch::dtype(torch::kInt64).device(region.device()));
  }
};

template <typename Launch>
c10::optional<torch::Tensor> msg_engine_v(const char* who, Launch launch,
                                          torch::Tensor region,
                                          torch::Tensor offs,
                                          torch::Tensor addrs,
                                          torch::Tensor lens,
                                          int64_t max_msg_bytes, bool crc,
                                          int64_t grid_cap) {
  OnDeviceOf dev(region, who);
  VarLenArgs a(who, region, offs, &addrs, lens, max_msg_bytes, grid_cap);
  c10::optional<torch::Tensor> out;
  if (crc)
    out = torch::empty({a.n},
                       torch::dtype(torch::kInt32).device(region.device()));
  HIP_OK(launch(region.data_ptr(), (const uint64_t*)offs.data_ptr<int64_t>(),
                (const uint64_t*)addrs.data_ptr<int64_t>(),
                (const uint64_t*)lens.data_ptr<int64_t>(), (uint32_t)a.n,
                (uint64_t)max_msg_bytes,
                (uint64_t*)a.cstart.data_ptr<int64_t>(),
                crc ? (uint32_t*)out->data_ptr<int32_t>() : nullptr,
                (uint32_t)grid_cap, dev.stream));
  return out;
}

c10::optional<torch::Tensor> gather_v_(torch::Tensor region,
                                       torch::Tensor dst_offs,
                                       torch::Tensor src_addrs,
                                       torch::Tensor lens,
                                       int64_t max_msg_bytes, bool crc,
                                       int64_t grid_cap) {
  return msg_engine_v("gather_v_", rocp2p_gather_v, region, dst_offs,
                      src_addrs, lens, max_msg_bytes, crc, grid_cap);
}

c10::optional<torch::Tensor> scatter_v_(torch::Tensor region,
                                        torch::Tensor src_offs,
                                        torch::Tensor dst_addrs,
                                        torch::Tensor lens,
                                        int64_t max_msg_bytes, bool crc,
                                        int64_t grid_cap) {
  return msg_engine_v("scatter_v_", rocp2p_scatter_v, region, src_offs,
                      dst_addrs, lens, max_msg_bytes, crc, grid_cap);
}

torch::Tensor crc32_messages_v(torch::Tensor region, torch::Tensor offs,
                               torch::Tensor lens, int64_t max_msg_bytes,
                               int64_t grid_cap) {
  OnDeviceOf dev(region, "crc32_messages_v");
  VarLenArgs a("crc32_messages_v", region, offs, nullptr, lens,
               max_msg_bytes, grid_cap);
  auto out = torch::empty({a.n},
                          torch::dtype(torch::kInt32).device(region.device()));
  HIP_OK(rocp2p_crc32_msgs_v(
      region.data_ptr(), (const uint64_t*)offs.data_ptr<int64_t>(),
      (const uint64_t*)lens.data_ptr<int64_t>(), (uint32_t)a.n,
      (uint64_t)max_msg_bytes, (uint64_t*)a.cstart.data_ptr<int64_t>(),
      (uint32_t*)out.data_ptr<int32_t>(), (uint32_t)grid_cap, dev.stream));
  return out;
}

// The byte-granular forms: any length at any address (p2p_bytes.h).
// Same host-visible checks as the _v forms — only the region base has
// to be 16-byte aligned — and the same scratch and digest tensors.
c10::optional<torch::Tensor> gather_bytes_(torch::Tensor region,
                                           torch::Tensor dst_offs,
                                           torch::Tensor src_addrs,
                                           torch::Tensor lens,
                                           int64_t max_msg_bytes, bool crc,
                                           int64_t grid_cap) {
  return msg_engine_v("gather_bytes_", rocp2p_gather_b, region, dst_offs,
                      src_addrs, lens, max_msg_bytes, crc, grid_cap);
}

c10::optional<torch::Tensor> scatter_bytes_(torch::Tensor region,
                                            torch::Tensor src_offs,
                                            torch::Tensor dst_addrs,
                                            torch::Tensor lens,
                                            int64_t max_msg_bytes, bool crc,
                                            int64_t grid_cap) {
  return msg_engine_v("scatter_bytes_", rocp2p_scatter_b, region, src_offs,
                      dst_addrs, lens, max_msg_bytes, crc, grid_cap);
}

torch::Tensor crc32_messages_bytes(torch::Tensor region, torch::Tensor offs,
                                   torch::Tensor lens, int64_t max_msg_bytes,
                                   int64_t grid_cap) {
  OnDeviceOf dev(region, "crc32_messages_bytes");
  VarLenArgs a("crc32_messages_bytes", region, offs, nullptr, lens,
               max_msg_bytes, grid_cap);
  auto out = torch::empty({a.n},
                          torch::dtype(torch::kInt32).device(region.device()));
  HIP_OK(rocp2p_crc32_msgs_b(
      region.data_ptr(), (const uint64_t*)offs.data_ptr<int64_t>(),
      (const uint64_t*)lens.data_ptr<int64_t>(), (uint32_t)a.n,
      (uint64_t)max_msg_bytes, (uint64_t*)a.cstart.data_ptr<int64_t>(),
      (uint32_t*)out.data_ptr<int32_t>(), (uint32_t)grid_cap, dev.stream));
  return out;
}

// The scatter/gather forms (p2p_sgl.h): every host-visible argument
// error raises before anything is launched; the scan scratch and the
// digests are torch tensors like the _v forms'.
template <typename Launch>
c10::optional<torch::Tensor> msg_engine_sg(
    const char* who, Launch launch, torch::Tensor region, torch::Tensor offs,
    torch::Tensor sge_start, torch::Tensor sge_addrs, torch::Tensor sge_lens,
    int64_t max_msg_bytes, bool crc, int64_t grid_cap) {
  OnDeviceOf dev(region, who);
  check_align16(region, who);
  for (const torch::Tensor* t : {&offs, &sge_start, &sge_addrs, &sge_lens}) {
    check_u64_dev(*t, who);
    TORCH_CHECK(t->device() == region.device(), who,
                ": descriptors must live on the region's device");
  }
  const int64_t n = offs.numel(), nsge = sge_lens.numel();
  TORCH_CHECK(sge_start.numel() == n + 1, who,
              ": sge_start must have n + 1 entries");
  TORCH_CHECK(sge_addrs.numel() == nsge, who,
              ": sge_addrs and sge_lens differ in length");
  TORCH_CHECK(n < (1LL << 32) && nsge < (1LL << 32), who,
              ": too many messages or SGEs");
  TORCH_CHECK(max_msg_bytes >= 0, who, ": max_msg_bytes out of range");
  TORCH_CHECK(grid_cap >= 0 && grid_cap <= 0xffffffffLL, who,
              ": grid_cap out of range");
  auto scratch = torch::empty(
      {(int64_t)ROCP2P_SGL_SCRATCH_WORDS(n, nsge)},
      torch::dtype(torch::kInt64).device(region.device()));
  c10::optional<torch::Tensor> out;
  if (crc)
    out = torch::empty({n},
                       torch::dtype(torch::kInt32).device(region.device()));
  HIP_OK(launch(region.data_ptr(), (const uint64_t*)offs.data_ptr<int64_t>(),
                (const uint64_t*)sge_start.data_ptr<int64_t>(),
                (const uint64_t*)sge_addrs.data_ptr<int64_t>(),
                (const uint64_t*)sge_lens.data_ptr<int64_t>(), (uint32_t)n,
                (uint32_t)nsge, (uint64_t)max_msg_bytes,
                (uint64_t*)scratch.data_ptr<int64_t>(),
                crc ? (uint32_t*)out->data_ptr<int32_t>() : nullptr,
                (uint32_t)grid_cap, dev.stream));
  return out;
}

c10::optional<torch::Tensor> gather_sg_(torch::Tensor region,
                                        torch::Tensor dst_offs,
                                        torch::Tensor sge_start,
                                        torch::Tensor sge_addrs,
                                        torch::Tensor sge_lens,
                                        int64_t max_msg_bytes, bool crc,
                                        int64_t grid_cap) {
  return msg_engine_sg("gather_sg_", rocp2p_gather_sg, region, dst_offs,
                       sge_start, sge_addrs, sge_lens, max_msg_bytes, crc,
                       grid_cap);
}

c10::optional<torch::Tensor> scatter_sg_(torch::Tensor region,
                                         torch::Tensor src_offs,
                                         torch::Tensor sge_start,
                                         torch::Tensor sge_addrs,
                                         torch::Tensor sge_lens,
                                         int64_t max_msg_bytes, bool crc,
                                         int64_t grid_cap) {
  return msg_engine_sg("scatter_sg_", rocp2p_scatter_sg, region, src_offs,
                       sge_start, sge_addrs, sge_lens, max_msg_bytes, crc,
                       grid_cap);
}

// The protected forms (p2p_prot.h): the checks of gather_bytes_, the key
// row, the MR table and the optional queue-pair word — every
// host-visible argument error raises before anything is launched.
// Status, scratch and digests are torch tensors like the _v forms'.
template <typename Launch>
std::tuple<torch::Tensor, c10::optional<torch::Tensor>> msg_engine_prot(
    const char* who, Launch launch, torch::Tensor region, torch::Tensor offs,
    torch::Tensor addrs, torch::Tensor lens, torch::Tensor keys,
    torch::Tensor mrs, c10::optional<torch::Tensor> qp_state,
    int64_t max_msg_bytes, bool crc, int64_t grid_cap) {
  OnDeviceOf dev(region, who);
  check_align16(region, who);
  for (const torch::Tensor* t : {&offs, &addrs, &lens, &keys, &mrs}) {
    check_u64_dev(*t, who);
    TORCH_CHECK(t->device() == region.device(), who,
                ": descriptors must live on the region's device");
  }
  const int64_t n = offs.numel();
  TORCH_CHECK(addrs.numel() == n && lens.numel() == n && keys.numel() == n,
              who, ": n mismatch");
  TORCH_CHECK(n < (1LL << 32), who, ": too many messages");
  TORCH_CHECK(mrs.dim() == 2 && mrs.size(1) == ROCP2P_PROT_MR_WORDS, who,
              ": mrs must have shape [R, 4] (key, addr, length, access)");
  TORCH_CHECK(mrs.size(0) >= 1 && mrs.size(0) <= (int64_t)ROCP2P_PROT_MAX_MR,
              who, ": mrs must have between 1 and 2^20 entries");
  int32_t* d_qp = nullptr;
  if (qp_state.has_value()) {
    TORCH_CHECK(qp_state->is_cuda() && qp_state->is_contiguous() &&
                    qp_state->scalar_type() == torch::kInt32 &&
                    qp_state->dim() == 1 && qp_state->numel() == 1,
                who, ": qp_state must be an int32 tensor of shape [1] on GPU");
    TORCH_CHECK(qp_state->device() == region.device(), who,
                ": qp_state must live on the region's device");
    d_qp = qp_state->data_ptr<int32_t>();
  }
  TORCH_CHECK(max_msg_bytes >= 0, who, ": max_msg_bytes out of range");
  TORCH_CHECK(grid_cap >= 0 && grid_cap <= 0xffffffffLL, who,
              ": grid_cap out of range");
  auto i32 = torch::dtype(torch::kInt32).device(region.device());
  auto status = torch::empty({n}, i32);
  auto scratch = torch::empty(
      {(int64_t)ROCP2P_PROT_SCRATCH_WORDS(n)},
      torch::dtype(torch::kInt64).device(region.device()));
  c10::optional<torch::Tensor> out;
  if (crc) out = torch::empty({n}, i32);
  if (!n) return {status, out};  // nothing to judge; the word stays
  HIP_OK(launch(region.data_ptr(), (const uint64_t*)offs.data_ptr<int64_t>(),
                (const uint64_t*)addrs.data_ptr<int64_t>(),
                (const uint64_t*)lens.data_ptr<int64_t>(),
                (const uint64_t*)keys.data_ptr<int64_t>(), (uint32_t)n,
                (const uint64_t*)mrs.data_ptr<int64_t>(),
                (uint32_t)mrs.size(0), d_qp, (uint64_t)max_msg_bytes,
                (uint64_t*)scratch.data_ptr<int64_t>(),
                status.data_ptr<int32_t>(),
                crc ? (uint32_t*)out->data_ptr<int32_t>() : nullptr,
                (uint32_t)grid_cap, dev.stream));
  return {status, out};
}

std::tuple<torch::Tensor, c10::optional<torch::Tensor>> gather_prot_(
    torch::Tensor region, torch::Tensor dst_offs, torch::Tensor src_addrs,
    torch::Tensor lens, torch::Tensor keys, torch::Tensor mrs,
    c10::optional<torch::Tensor> qp_state, int64_t max_msg_bytes, bool crc,
    int64_t grid_cap) {
  return msg_engine_prot("gather_prot_", rocp2p_gather_p, region, dst_offs,
                         src_addrs, lens, keys, mrs, qp_state, max_msg_bytes,
                         crc, grid_cap);
}

std::tuple<torch::Tensor, c10::optional<torch::Tensor>> scatter_prot_(
    torch::Tensor region, torch::Tensor src_offs, torch::Tensor dst_addrs,
    torch::Tensor lens, torch::Tensor keys, torch::Tensor mrs,
    c10::optional<torch::Tensor> qp_state, int64_t max_msg_bytes, bool crc,
    int64_t grid_cap) {
  return msg_engine_prot("scatter_prot_", rocp2p_scatter_p, region, src_offs,
                         dst_addrs, lens, keys, mrs, qp_state, max_msg_bytes,
                         crc, grid_cap);
}

void copy_(torch::Tensor dst, torch::Tensor src) {
  OnDeviceOf dev(dst, "copy_");
  check_buf(src, "copy_");
  TORCH_CHECK(nbytes_of(dst) == nbytes_of(src), "copy_: size mismatch");
  HIP_OK(rocp2p_copy(dst.data_ptr(), src.data_ptr(), nbytes_of(dst),
                     dev.stream));
}

void copy_nt_(torch::Tensor dst, torch::Tensor src) {
  OnDeviceOf dev(dst, "copy_nt_");
  check_buf(src, "copy_nt_");
  TORCH_CHECK(nbytes_of(dst) == nbytes_of(src), "copy_nt_: size mismatch");
  HIP_OK(rocp2p_copy_nt(dst.data_ptr(), src.data_ptr(), nbytes_of(dst),
                        dev.stream));
}

// Export an HBM range as a dmabuf fd — the GPU half of the verbs
// backend's kernel-module-free MR mode (ibv_reg_dmabuf_mr); lets a
// GPU-only box validate that machinery without an HCA.  Caller owns
// the fd (os.close it).
int64_t dmabuf_fd(torch::Tensor buf) {
  OnDeviceOf dev(buf, "dmabuf_fd");
  int fd = -1;
  hipError_t e = hipMemGetHandleForAddressRange(
      &fd, buf.data_ptr(), nbytes_of(buf), hipMemRangeHandleTypeDmaBufFd,
      0);
  TORCH_CHECK(e == hipSuccess, "hipMemGetHandleForAddressRange: ",
              hipGetErrorString(e));
  return fd;
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "MI355X payload kernels: splitmix64 fill / verify, per-page, "
            "per-message and whole-region CRC32, streaming copy";
  m.def("fill_", &fill_, "in-place splitmix64 pattern fill");
  m.def("verify", &verify, "count words deviating from the pattern");
  m.def("crc32_pages", &crc32_pages, "zlib CRC32 of each 4 KiB page");
  m.def("crc32_messages", &crc32_messages,
        "zlib CRC32 of each msg_bytes message (optionally at offs)",
        py::arg("region"), py::arg("msg_bytes"),
        py::arg("offs") = py::none(), py::arg("grid_cap") = 0);
  m.def("crc32", &crc32, "zlib CRC32 of a whole buffer, any byte length",
        py::arg("buf"), py::arg("grid_cap") = 0);
  m.def("copy_", &copy_, "streaming device copy dst <- src");
  m.def("copy_nt_", &copy_nt_, "nontemporal streaming device copy");
  m.def("gather_", &gather_,
        "batched message engine: host-pinned srcs -> HBM region offsets");
  m.def("scatter_", &scatter_,
        "batched message engine: HBM region offsets -> host-pinned dsts");
  m.def("gather_crc_", &gather_crc_,
        "gather_ plus one zlib CRC32 per message, taken in the same pass",
        py::arg("region"), py::arg("dst_offs"), py::arg("src_addrs"),
        py::arg("msg_bytes"), py::arg("grid_cap") = 0);
  m.def("scatter_crc_", &scatter_crc_,
        "scatter_ plus one zlib CRC32 per message, taken in the same pass",
        py::arg("region"), py::arg("src_offs"), py::arg("dst_addrs"),
        py::arg("msg_bytes"), py::arg("grid_cap") = 0);
  m.def("gather_v_", &gather_v_,
        "gather_ for per-message lengths; crc=True adds the inline ICRC",
        py::arg("region"), py::arg("dst_offs"), py::arg("src_addrs"),
        py::arg("lens"), py::arg("max_msg_bytes") = 0,
        py::arg("crc") = false, py::arg("grid_cap") = 0);
  m.def("scatter_v_", &scatter_v_,
        "scatter_ for per-message lengths; crc=True adds the inline ICRC",
        py::arg("region"), py::arg("src_offs"), py::arg("dst_addrs"),
        py::arg("lens"), py::arg("max_msg_bytes") = 0,
        py::arg("crc") = false, py::arg("grid_cap") = 0);
  m.def("crc32_messages_v", &crc32_messages_v,
        "zlib CRC32 of each message base[offs[m], offs[m] + lens[m])",
        py::arg("region"), py::arg("offs"), py::arg("lens"),
        py::arg("max_msg_bytes") = 0, py::arg("grid_cap") = 0);
  m.def("gather_bytes_", &gather_bytes_,
        "gather_v_ for any byte length at any byte address",
        py::arg("region"), py::arg("dst_offs"), py::arg("src_addrs"),
        py::arg("lens"), py::arg("max_msg_bytes") = 0,
        py::arg("crc") = false, py::arg("grid_cap") = 0);
  m.def("scatter_bytes_", &scatter_bytes_,
        "scatter_v_ for any byte length at any byte address",
        py::arg("region"), py::arg("src_offs"), py::arg("dst_addrs"),
        py::arg("lens"), py::arg("max_msg_bytes") = 0,
        py::arg("crc") = false, py::arg("grid_cap") = 0);
  m.def("crc32_messages_bytes", &crc32_messages_bytes,
        "crc32_messages_v for offsets of any alignment",
        py::arg("region"), py::arg("offs"), py::arg("lens"),
        py::arg("max_msg_bytes") = 0, py::arg("grid_cap") = 0);
  m.def("gather_sg_", &gather_sg_,
        "gather_bytes_ for messages that are lists of outside buffers (CSR)",
        py::arg("region"), py::arg("dst_offs"), py::arg("sge_start"),
        py::arg("sge_addrs"), py::arg("sge_lens"),
        py::arg("max_msg_bytes") = 0, py::arg("crc") = false,
        py::arg("grid_cap") = 0);
  m.def("scatter_sg_", &scatter_sg_,
        "scatter_bytes_ for messages that are lists of outside buffers (CSR)",
        py::arg("region"), py::arg("src_offs"), py::arg("sge_start"),
        py::arg("sge_addrs"), py::arg("sge_lens"),
        py::arg("max_msg_bytes") = 0, py::arg("crc") = false,
        py::arg("grid_cap") = 0);
  m.def("gather_prot_", &gather_prot_,
        "gather_bytes_ behind MR keys, bounds and access checks; returns "
        "(status, digests or None)",
        py::arg("region"), py::arg("dst_offs"), py::arg("src_addrs"),
        py::arg("lens"), py::arg("keys"), py::arg("mrs"),
        py::arg("qp_state") = py::none(), py::arg("max_msg_bytes") = 0,
        py::arg("crc") = false, py::arg("grid_cap") = 0);
  m.def("scatter_prot_", &scatter_prot_,
        "scatter_bytes_ behind MR keys, bounds and access checks; returns "
        "(status, digests or None)",
        py::arg("region"), py::arg("src_offs"), py::arg("dst_addrs"),
        py::arg("lens"), py::arg("keys"), py::arg("mrs"),
        py::arg("qp_state") = py::none(), py::arg("max_msg_bytes") = 0,
        py::arg("crc") = false, py::arg("grid_cap") = 0);
  m.def("dmabuf_fd", &dmabuf_fd,
        "export an HBM tensor range as a dmabuf fd (caller closes)");
}
