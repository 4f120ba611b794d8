// A ring of pinned host slots in front of one copy stream: the caller's (pageable, possibly read-only) memory crosses PCIe in
// pieces of at most slot_words words without ever being pinned itself.  Per piece the caller
//   claim()s the next slot -- the host waits here until the copy that last left that slot has completed, so it runs at most
//            `slots` pieces ahead of the copy engine --
//   fills it, issues its own hipMemcpyAsync out of it (and whatever stream waits it needs in front), and
//   sent() records the slot's event behind that copy.
// The slots rotate in claim order and the rotation carries over from call to call; a caller that drains the stream between calls
// finds every slot free.  The methods return hipError_t: each caller wraps them in its own error macro and message.  Used by the
// trace loads of a prover (trace_load.hip: 4 slots of 16 MiB, created on first use) and by the batch verifier
// (verifier_device.hip: 4 slots of 4 MiB, created with the verifier).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

struct PinnedRing {
  static constexpr unsigned MAX_SLOTS = 4;
  uint64_t* base = nullptr;             // [slots][slot_words], pinned
  size_t slot_words = 0;
  unsigned slots = 0, next = 0;
  hipEvent_t copied[MAX_SLOTS] = {};    // copy stream: the copy out of slot s has completed
  bool used[MAX_SLOTS] = {};

  // idempotent: a call that failed half way is completed by the next one
  hipError_t create(unsigned nslots, size_t words) {
    if (nslots > MAX_SLOTS) return hipErrorInvalidValue;
    slots = nslots; slot_words = words;
    for (unsigned s = 0; s < slots; s++)
      if (!copied[s]) if (hipError_t e = hipEventCreateWithFlags(&copied[s], hipEventDisableTiming)) return e;
    if (!base) return hipHostMalloc((void**)&base, (size_t)slots * slot_words * sizeof(uint64_t), hipHostMallocDefault);
    return hipSuccess;
  }
  void destroy() {   // (a partly created ring holds null handles)
    for (auto& e : copied) if (e) { (void)hipEventDestroy(e); e = nullptr; }
    if (base) { (void)hipHostFree(base); base = nullptr; }
  }
  hipError_t claim(uint64_t** slot, unsigned* s) {
    *s = next; next = (next + 1) % slots;
    *slot = base + (size_t)*s * slot_words;
    return used[*s] ? hipEventSynchronize(copied[*s]) : hipSuccess;
  }
  hipError_t sent(unsigned s, hipStream_t stream) {
    const hipError_t e = hipEventRecord(copied[s], stream);
    if (e == hipSuccess) used[s] = true;
    return e;
  }
};
