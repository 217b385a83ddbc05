// stage_common.h -- the host-side plumbing the timestep-end stages (stage_spectra.h, stage_radfield.h, stage_ionbal.h) share:
// the error return, the struct_size check, the optional copy and the one device block a stage carves its arrays from.
// Included by artis_engine.hip after the engine struct (HIP_TRY, g_last_error).
#pragma once

namespace {

// every stage's error return: the text is "<stage>: <what>" (callers and tests read it)
int stage_error(int code, const std::string &msg) {
  g_last_error = msg;
  return code;
}

// a caller's struct was built against this header
#define STAGE_STRUCT_SIZE(p, T, stage) \
  if ((p)->struct_size != (int64_t)sizeof(T)) return stage_error(ARTIS_ERR_ARG, stage ": " #T ".struct_size does not match")

// copy count elements, unless an array is absent (null) or empty; on *stream without waiting when one is given. (The cell state's
// arrays are pointers to const: the hand-over writes them.)
template <class D, class S>
hipError_t stage_copy(D *dst, const S *src, int64_t count, hipMemcpyKind kind, const hipStream_t *stream = nullptr) {
  static_assert(sizeof(D) == sizeof(S), "stage_copy: element sizes differ");
  if (!dst || !src || count <= 0) return hipSuccess;
  void *to = const_cast<std::remove_const_t<D> *>(dst);
  return stream ? hipMemcpyAsync(to, src, sizeof(S) * (size_t)count, kind, *stream) : hipMemcpy(to, src, sizeof(S) * (size_t)count, kind);
}

// one array of a stage's block: where its pointer goes, how many elements of what size
struct StagePiece {
  void **ptr;
  int64_t count;
  size_t elem;
};
template <class T>
StagePiece piece(T **ptr, int64_t count) {
  return {(void **)ptr, count, sizeof(T)};
}

// One device allocation holding every array of a stage (256-byte aligned pieces; an empty piece gets a null pointer), zeroed when
// made, with the events the stage times its kernels by. Freed with the state that owns it.
struct StageBlock {
  void *base = nullptr;
  size_t bytes = 0;
  hipEvent_t ev[4] = {};

  // `what` names the block in the error texts ("radfield: the result block"); it must fit 90 % of the free device memory
  int make(const std::vector<StagePiece> &pieces, const std::string &stage, const std::string &what) {
    bytes = carve(pieces, nullptr);
    size_t free_b = 0, total_b = 0;
    hipError_t err = hipMemGetInfo(&free_b, &total_b);
    if (err == hipSuccess && (double)bytes > 0.9 * (double)free_b)
      return stage_error(ARTIS_ERR_ARG, stage + ": " + what + " does not fit the free device memory");
    if (err == hipSuccess) err = hipMalloc(&base, bytes);
    if (err == hipSuccess) err = hipMemset(base, 0, bytes);
    for (hipEvent_t &e : ev)
      if (err == hipSuccess) err = hipEventCreate(&e);
    if (err != hipSuccess) return stage_error(ARTIS_ERR_HIP, stage + ": allocation of " + what + ": " + hipGetErrorString(err));
    carve(pieces, (char *)base);
    return ARTIS_OK;
  }
  // milliseconds between events k and k + 1
  hipError_t elapsed_ms(int k, double *ms) const {
    float f = 0.f;
    const hipError_t err = hipEventElapsedTime(&f, ev[k], ev[k + 1]);
    *ms = f;
    return err;
  }
  ~StageBlock() {
    if (base) (void)hipFree(base);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }

 private:
  // with at == nullptr only the size is counted
  static size_t carve(const std::vector<StagePiece> &pieces, char *at) {
    size_t off = 0;
    for (const StagePiece &p : pieces) {
      if (at) *p.ptr = p.count > 0 ? at + off : nullptr;
      off += ((size_t)(p.count > 0 ? p.count : 0) * p.elem + 255) & ~(size_t)255;
    }
    return off;
  }
};

}  // namespace
