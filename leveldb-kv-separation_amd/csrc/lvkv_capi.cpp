// C-ABI of the batched CRC32C engine (declarations: include/lvkv_crc32c.h).
//
// Device state per HIP device (tables, CU count, staging for the host API) is
// created once, lazily, under std::call_once; the per-call paths take no lock
// and allocate nothing, so device-resident calls can be captured in a graph.
// Errors are return codes: this library backs a -fno-exceptions caller
// (reference CMakeLists.txt:71-77) and never throws or aborts.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <unordered_map>
#include <mutex>
#include <thread>
#include <vector>

#include "crc32c_modes.h"
#include "lvkv_crc32c.h"
#include "lvkv_kernel_args.h"
#include "lvkv_launch.h"
#include "lvkv_scratch.h"
#include "lvkv_snappy.h"
#include "lvkv_tables.h"

namespace lvkv {

namespace {

constexpr int kMaxDevices = 64;
// Blocks per launch: the kernel indexes blocks with u32.
constexpr size_t kMaxBlocksPerLaunch = size_t{1} << 30;

// Host-API staging (double-buffered chunks).
constexpr size_t kStageBytes = size_t{64} << 20;
constexpr size_t kStageBlocks = 1u << 16;

struct Stage {
  uint8_t* h_data = nullptr;  // pinned
  uint8_t* d_data = nullptr;
  size_t cap = 0;
  uint64_t* h_off = nullptr;  // pinned descriptors
  uint32_t* h_len = nullptr;
  uint32_t* h_init = nullptr;
  uint32_t* h_out = nullptr;
  uint64_t* d_off = nullptr;
  uint32_t* d_len = nullptr;
  uint32_t* d_init = nullptr;
  uint32_t* d_out = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;
  size_t first = 0, count = 0;  // blocks of the batch held by this stage
  bool busy = false;
};

struct DeviceCtx {
  std::once_flag once;
  int status = LVKV_ERR_NO_DEVICE;
  int groups = 0;  // one workgroup per CU
  uint32_t* d_tables = nullptr;
  uint32_t zcol[32];  // columns of Z_256 (uniform kernel's row tables)
  // kernels of general-layout batches and of WAL records
  // (launch_crc32c_general; lvkv_debug_set_general_kernel/_log_kernel)
  std::atomic<int> general_cfg{0};  // ragged cfg 0: 8 waves x 2 chains x 24 rows
  std::atomic<int> log_cfg{8};      // one workgroup per round of 32 small records
  // whole-SSTable verify form: 0 by size, 1 fused, 2 two launches,
  // 3 speculative (lvkv_debug_set_sst_form)
  std::atomic<int> sst_form{0};
  std::mutex host_mu;  // serialises lvkv_crc32c_batch_host per device
  // WAL verify scratch: a pool of buffers, each lent to one call at a time
  // (busy from acquire to the event recorded after the call's launches,
  // free once that event completes), on any stream
  std::mutex scratch_mu;
  struct Scratch {
    void* p = nullptr;
    size_t bytes = 0;
    hipEvent_t ev = nullptr;
    hipStream_t stream = nullptr;  // of its last call
    bool lent = false;
  };
  std::vector<Scratch> log_pool;
  bool stages_ready = false;
  Stage stage[2];
};

DeviceCtx g_dev[kMaxDevices];
thread_local int t_last_hip_error = 0;

int hip_fail(hipError_t e) {
  t_last_hip_error = static_cast<int>(e);
  return LVKV_ERR_HIP;
}

void init_ctx(DeviceCtx& c, int dev) {
  int ncu = 0;
  hipError_t e =
      hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
  if (e != hipSuccess || ncu <= 0) {
    c.status = hip_fail(e);
    return;
  }
  static_assert(kZPowOffset == kRowTabDwords + kLaneTabDwords + kLaneColDwords, "layout");
  std::vector<uint32_t> tab(kTableDwords);
  build_row_table(tab.data());
  build_lane_table(tab.data() + kRowTabDwords);
  build_lane_columns(tab.data() + kRowTabDwords + kLaneTabDwords);
  build_zpow_tables(tab.data() + kZPowOffset);
  build_zmul_columns(tab.data() + kZPowOffset + kZPowDwords);
  void* p = nullptr;
  e = hipMalloc(&p, tab.size() * sizeof(uint32_t));
  if (e != hipSuccess) {
    c.status = hip_fail(e);
    return;
  }
  e = hipMemcpy(p, tab.data(), tab.size() * sizeof(uint32_t),
                hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(p);
    c.status = hip_fail(e);
    return;
  }
  c.d_tables = static_cast<uint32_t*>(p);
  const Gf2Op z256 = gf2_zero_advance(kRowBytes);
  for (int b = 0; b < 32; ++b) c.zcol[b] = z256.col[b];
  c.groups = ncu;
  c.status = LVKV_OK;
}

DeviceCtx* current_ctx(int* rc) {
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0) {
    t_last_hip_error = static_cast<int>(e);
    *rc = LVKV_ERR_NO_DEVICE;
    return nullptr;
  }
  int dev = -1;
  e = hipGetDevice(&dev);
  if (e != hipSuccess) {
    *rc = hip_fail(e);
    return nullptr;
  }
  if (dev < 0 || dev >= kMaxDevices) {
    *rc = LVKV_ERR_INVALID;
    return nullptr;
  }
  DeviceCtx& c = g_dev[dev];
  std::call_once(c.once, [&] { init_ctx(c, dev); });
  *rc = c.status;
  return c.status == LVKV_OK ? &c : nullptr;
}

}  // namespace

// The current device's tables (lvkv_engine.cpp shares them).
uint32_t* device_tables(int* rc) {
  DeviceCtx* c = current_ctx(rc);
  return c != nullptr ? c->d_tables : nullptr;
}

namespace {

UniformArgs uniform_args(const DeviceCtx& c, const KernelArgs& b) {
  UniformArgs u;
  memset(&u, 0, sizeof(u));
  u.base = b.base;
  u.stride = b.stride;
  u.out = b.out_crc;
  u.lane_tab = c.d_tables + kRowTabDwords;
  u.lane_cols = c.d_tables + kRowTabDwords + kLaneTabDwords;
  u.stamps = b.stamps;
  u.zpow = c.d_tables + kZPowOffset;
  u.length = b.length;
  u.init = b.init;
  u.nblocks = b.nblocks;
  u.mask = b.mask;
  memcpy(u.zcol, c.zcol, sizeof(u.zcol));
  return u;
}

int run_batch(KernelArgs a, size_t nblocks, hipStream_t stream) {
  if (nblocks == 0) return LVKV_OK;
  int rc = LVKV_OK;
  DeviceCtx* c = current_ctx(&rc);
  if (c == nullptr) return rc;
  a.row_tab = c->d_tables;
  a.lane_tab = c->d_tables + kRowTabDwords;
  a.general_cfg = c->general_cfg.load(std::memory_order_relaxed);
  a.log_cfg = c->log_cfg.load(std::memory_order_relaxed);
  for (size_t done = 0; done < nblocks;) {
    const size_t n = std::min(nblocks - done, kMaxBlocksPerLaunch);
    KernelArgs b = a;
    b.nblocks = static_cast<uint32_t>(n);
    if (a.offsets != nullptr) {
      b.offsets = a.offsets + done;
      if (a.lengths != nullptr) b.lengths = a.lengths + done;
    } else {
      b.base = a.base + done * a.stride;
    }
    if (a.inits != nullptr) b.inits = a.inits + done;
    if (a.out_crc != nullptr) b.out_crc = a.out_crc + done;
    if (a.out_status != nullptr) b.out_status = a.out_status + done;
    const size_t want = (n + kWavesPerGroup - 1) / kWavesPerGroup;
    const int groups = static_cast<int>(
        std::min<size_t>(static_cast<size_t>(c->groups), want));
    // Uniform layout whose every block END is 4-byte aligned: the dedicated
    // uniform kernel (crc32c_uniform.hip).
    const bool uni_aligned =
        a.offsets == nullptr && a.mode == kModeCompute && a.length >= 4 &&
        (a.stride % 4) == 0 &&
        ((reinterpret_cast<uintptr_t>(b.base) + a.length) % 4) == 0;
    hipError_t e;
    if (uni_aligned) {
      // Blocks of <= 16 rows (4 KiB + 252 B) that fit one round of the
      // compact-LDS kernel (two 512-thread workgroups per CU, 24 blocks
      // each): crc32c_compact.hip. At least 3 blocks per workgroup.
      const int cgroups = static_cast<int>(std::min<size_t>(
          static_cast<size_t>(c->groups) * compact_occupancy(kCompactProductionCfg),
          (n + 2) / 3));
      const size_t waves = static_cast<size_t>(groups) * kWavesPerGroup;
      if (a.length <= kRowsPerChunk * kRowBytes &&
          n <= static_cast<size_t>(cgroups) * compact_capacity(kCompactProductionCfg))
        e = launch_crc32c_compact(uniform_args(*c, b), kCompactProductionCfg, cgroups, stream);
      // One round per wave when every wave owns <= 3 single-chunk blocks.
      else if (a.length <= kRowsPerChunk * kRowBytes && n <= 3 * waves)
        e = launch_crc32c_uniform_small(uniform_args(*c, b), kSmallProductionVariant,
                                        groups, stream);
      else
        e = launch_crc32c_uniform(uniform_args(*c, b), 0, groups, stream);
    } else if (b.offsets != nullptr) {
      // Blocks longer than the mode's bound go to one workgroup each
      // (segments in parallel) instead of one wave.
      b.long_split = mode_long_split(b.mode);
      e = launch_crc32c_general(b, c->groups, stream);
    } else {  // uniform layout, block ends not 4-byte aligned
      e = launch_crc32c_batch(b, false, groups, stream);
    }
    if (e != hipSuccess) return hip_fail(e);
    done += n;
  }
  return LVKV_OK;
}

// "filter." + policy name (table.cc:100-101); false if the name is too long.
bool filter_key(const char* policy, FilterKey* fk) {
  memset(fk, 0, sizeof(*fk));
  if (policy == nullptr) return true;  // no filter policy: no filter block
  const size_t n = strlen(policy);
  if (n > LVKV_SST_MAX_POLICY_NAME) return false;
  memcpy(fk->key, "filter.", 7);
  memcpy(fk->key + 7, policy, n);
  fk->len = static_cast<uint32_t>(7 + n);
  return true;
}

// The one-launch SST verify forms for one table up to this size (larger
// indexes are faster on the two-launch form's 16-wave heads and its wide
// index launch). Multi-table calls take the speculative form (each CRC
// workgroup decodes its own share of one table's index) up to half as many
// tables as CUs, the two launches beyond.
constexpr uint64_t kFusedTableBytes = uint64_t{32} << 20;
constexpr size_t kFusedMaxTables = 256;

// kSstForm* for a call: lvkv_debug_set_sst_form's 1 (fused), 2 (two
// launches), 3 (speculative), or by size (0). The speculative form needs
// fewer tables than half its grid.
int sst_form(const DeviceCtx& c, bool by_size, size_t ntables = 1) {
  const int mode = c.sst_form.load(std::memory_order_relaxed);
  const bool spec_ok = ntables * 2 <= static_cast<size_t>(c.groups);
  switch (mode) {
    case 1: return ntables <= kFusedMaxTables ? kSstFormFused : kSstFormTwo;
    case 2: return kSstFormTwo;
    case 3: return spec_ok ? kSstFormSpec : kSstFormTwo;
  }
  return by_size && spec_ok ? kSstFormSpec : kSstFormTwo;
}

// Per-call tag of the multi-table placement words (never 0: fresh report
// memory is often zeroed).
uint32_t next_sst_generation() {
  static std::atomic<uint32_t> g{0};
  uint32_t v;
  do {
    v = g.fetch_add(1, std::memory_order_relaxed) + 1;
  } while (v == 0);
  return v;
}

KernelArgs blank_args() {
  KernelArgs a;
  memset(&a, 0, sizeof(a));
  return a;
}

// Zeroed arguments with the device context's tables and kernel choices.
KernelArgs ctx_args(const DeviceCtx& c) {
  KernelArgs a = blank_args();
  a.row_tab = c.d_tables;
  a.lane_tab = c.d_tables + kRowTabDwords;
  a.general_cfg = c.general_cfg.load(std::memory_order_relaxed);
  a.log_cfg = c.log_cfg.load(std::memory_order_relaxed);
  return a;
}

// A WAL verify scratch buffer of at least `bytes` for one call on `stream`.
// A buffer whose last call has finished (its event completed; never
// recorded counts as completed) is taken as is; else one last used on this
// same stream, or, with four buffers in the pool, any big enough idle one, is
// taken behind its event (hipStreamWaitEvent: the new call starts after the
// old one ends, a no-op on the same stream). When none is big enough, an idle
// buffer is regrown in place (after its last call has ended: its event is
// synchronised before the free) or, below four buffers, one is added; the
// pool exceeds four only while every buffer is lent to a call in progress on
// another thread. A new buffer's counters (bytes [0, 32)) are zeroed on
// `stream`; every call leaves them at 0. Not capturable: a graph would replay
// the counters unzeroed. The buffers live as long as the process (the HIP
// runtime may be gone by the time static destructors run).
hipError_t log_scratch_acquire(DeviceCtx& c, hipStream_t stream, size_t bytes, void** out,
                               size_t* slot) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  hipError_t e = hipStreamIsCapturing(stream, &cs);
  if (e != hipSuccess) return e;
  if (cs != hipStreamCaptureStatusNone) return hipErrorStreamCaptureUnsupported;
  std::unique_lock<std::mutex> lk(c.scratch_mu);
  constexpr size_t kPoolMax = 4;
  size_t same = SIZE_MAX, any = SIZE_MAX, idle_small = SIZE_MAX, busy_small = SIZE_MAX;
  for (size_t i = 0; i < c.log_pool.size(); ++i) {
    auto& b = c.log_pool[i];
    if (b.lent) continue;
    const bool finished = hipEventQuery(b.ev) == hipSuccess;
    if (b.bytes < bytes) {
      if (finished)
        idle_small = i;
      else
        busy_small = i;
      continue;
    }
    if (finished) {
      b.lent = true;
      b.stream = stream;
      *out = b.p;
      *slot = i;
      return hipSuccess;
    }
    if (b.stream == stream) same = i;
    any = i;
  }
  const bool full = c.log_pool.size() >= kPoolMax;
  size_t pick = same != SIZE_MAX ? same : (full ? any : SIZE_MAX);
  if (pick != SIZE_MAX) {
    auto& b = c.log_pool[pick];
    if ((e = hipStreamWaitEvent(stream, b.ev, 0)) != hipSuccess) return e;
    b.lent = true;
    b.stream = stream;
    *out = b.p;
    *slot = pick;
    return hipSuccess;
  }
  // nothing big enough: regrow an idle buffer (a busy one once its call has
  // ended) when the pool is full, else add one
  if (idle_small == SIZE_MAX && full) idle_small = busy_small;
  if (idle_small == SIZE_MAX) {
    DeviceCtx::Scratch n;
    if ((e = hipEventCreateWithFlags(&n.ev, hipEventDisableTiming)) != hipSuccess) return e;
    c.log_pool.push_back(n);
    idle_small = c.log_pool.size() - 1;
  }
  // Take the slot out of the pool, then wait for its last call and
  // reallocate without the lock: other streams' acquires and releases on
  // this device go on meanwhile (the slot is addressed by index, since the
  // pool may grow).
  const size_t k = idle_small;
  void* old = c.log_pool[k].p;
  const hipEvent_t ev = c.log_pool[k].ev;
  c.log_pool[k].lent = true;
  c.log_pool[k].p = nullptr;
  c.log_pool[k].bytes = 0;
  lk.unlock();
  const size_t cap = std::max<size_t>(bytes, size_t{1} << 16);
  void* p = nullptr;
  if (old != nullptr) {
    e = hipEventSynchronize(ev);
    if (e == hipSuccess) e = hipFree(old);
  }
  if (e == hipSuccess) e = hipMalloc(&p, cap);
  if (e == hipSuccess) e = hipMemsetAsync(p, 0, 32, stream);
  lk.lock();
  auto& b = c.log_pool[k];
  if (e != hipSuccess) {
    if (p != nullptr) (void)hipFree(p);
    b.lent = false;  // empty: the next acquire allocates it afresh
    return e;
  }
  b.p = p;
  b.bytes = cap;
  b.stream = stream;
  *out = p;
  *slot = k;
  return hipSuccess;
}

// Hands the buffer back: busy until the work just launched on `stream` ends.
hipError_t log_scratch_release(DeviceCtx& c, size_t slot, hipStream_t stream) {
  std::lock_guard<std::mutex> lk(c.scratch_mu);
  auto& b = c.log_pool[slot];
  const hipError_t e = hipEventRecord(b.ev, stream);
  b.lent = false;
  return e;
}

// ---- host-resident pipeline ------------------------------------------

void free_stage(Stage& s) {
  if (s.h_data) (void)hipHostFree(s.h_data);
  if (s.d_data) (void)hipFree(s.d_data);
  s.h_data = s.d_data = nullptr;
  s.cap = 0;
}

int alloc_stage_data(Stage& s, size_t cap) {
  free_stage(s);
  hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&s.h_data), cap,
                               hipHostMallocDefault);
  if (e != hipSuccess) return hip_fail(e);
  e = hipMalloc(reinterpret_cast<void**>(&s.d_data), cap);
  if (e != hipSuccess) return hip_fail(e);
  s.cap = cap;
  return LVKV_OK;
}

int ensure_stages(DeviceCtx& c, size_t need_bytes) {
  const size_t cap = std::max(kStageBytes, (need_bytes + 4095) & ~size_t{4095});
  for (Stage& s : c.stage) {
    if (!c.stages_ready) {
      hipError_t e;
      if ((e = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking)) !=
          hipSuccess)
        return hip_fail(e);
      if ((e = hipEventCreateWithFlags(&s.done, hipEventDisableTiming)) !=
          hipSuccess)
        return hip_fail(e);
      const size_t nb = kStageBlocks;
      if ((e = hipHostMalloc(reinterpret_cast<void**>(&s.h_off), nb * 8,
                             hipHostMallocDefault)) != hipSuccess ||
          (e = hipHostMalloc(reinterpret_cast<void**>(&s.h_len), nb * 4,
                             hipHostMallocDefault)) != hipSuccess ||
          (e = hipHostMalloc(reinterpret_cast<void**>(&s.h_init), nb * 4,
                             hipHostMallocDefault)) != hipSuccess ||
          (e = hipHostMalloc(reinterpret_cast<void**>(&s.h_out), nb * 4,
                             hipHostMallocDefault)) != hipSuccess ||
          (e = hipMalloc(reinterpret_cast<void**>(&s.d_off), nb * 8)) !=
              hipSuccess ||
          (e = hipMalloc(reinterpret_cast<void**>(&s.d_len), nb * 4)) !=
              hipSuccess ||
          (e = hipMalloc(reinterpret_cast<void**>(&s.d_init), nb * 4)) !=
              hipSuccess ||
          (e = hipMalloc(reinterpret_cast<void**>(&s.d_out), nb * 4)) !=
              hipSuccess)
        return hip_fail(e);
    }
    if (s.cap < cap) {
      int rc = alloc_stage_data(s, cap);
      if (rc != LVKV_OK) return rc;
    }
  }
  c.stages_ready = true;
  return LVKV_OK;
}

// Copy blocks into the pinned buffer; big chunks are split over threads.
void pack_parallel(uint8_t* dst, const uint8_t* src, const uint64_t* src_off,
                   const uint32_t* len, const uint64_t* dst_off, size_t n,
                   size_t bytes) {
  const size_t kPerThread = size_t{8} << 20;
  unsigned hw = std::thread::hardware_concurrency();
  size_t nt = std::min<size_t>(hw ? hw : 1, 16);
  nt = std::min(nt, std::max<size_t>(1, bytes / kPerThread));
  auto work = [&](size_t t) {
    for (size_t i = t; i < n; i += nt)
      memcpy(dst + dst_off[i], src + src_off[i], len[i]);
  };
  if (nt <= 1) {
    work(0);
    return;
  }
  std::vector<std::thread> th;
  for (size_t t = 1; t < nt; ++t) th.emplace_back(work, t);
  work(0);
  for (auto& x : th) x.join();
}

int drain_stage(Stage& s, uint32_t* h_out) {
  if (!s.busy) return LVKV_OK;
  hipError_t e = hipEventSynchronize(s.done);
  s.busy = false;
  if (e != hipSuccess) return hip_fail(e);
  memcpy(h_out + s.first, s.h_out, s.count * sizeof(uint32_t));
  return LVKV_OK;
}

}  // namespace
}  // namespace lvkv

using namespace lvkv;

extern "C" {

uint32_t lvkv_crc32c_extend(uint32_t init_crc, const char* data, size_t n) {
  return cpu_crc32c_extend(init_crc, reinterpret_cast<const uint8_t*>(data), n);
}

uint32_t lvkv_crc32c_value(const char* data, size_t n) {
  return cpu_crc32c_extend(0, reinterpret_cast<const uint8_t*>(data), n);
}

uint32_t lvkv_crc32c_mask(uint32_t crc) {
  return ((crc >> 15) | (crc << 17)) + kMaskDelta;
}

uint32_t lvkv_crc32c_unmask(uint32_t masked_crc) {
  const uint32_t r = masked_crc - kMaskDelta;
  return (r >> 17) | (r << 15);
}

int lvkv_crc32c_batch_device(const void* d_base, const uint64_t* d_offsets,
                             const uint32_t* d_lengths, const uint32_t* d_init,
                             uint32_t init, uint32_t* d_out, size_t nblocks,
                             uint32_t flags, void* stream) {
  if (nblocks == 0) return LVKV_OK;
  if (!d_base || !d_offsets || !d_lengths || !d_out) return LVKV_ERR_INVALID;
  KernelArgs a = blank_args();
  a.base = static_cast<const uint8_t*>(d_base);
  a.offsets = d_offsets;
  a.lengths = d_lengths;
  a.inits = d_init;
  a.init = init;
  a.out_crc = d_out;
  a.mode = kModeCompute;
  a.mask = (flags & LVKV_FLAG_MASK) ? 1u : 0u;
  return run_batch(a, nblocks, static_cast<hipStream_t>(stream));
}

int lvkv_crc32c_uniform_device(const void* d_base, uint64_t stride,
                               uint32_t length, uint32_t init, uint32_t* d_out,
                               size_t nblocks, uint32_t flags, void* stream) {
  if (nblocks == 0) return LVKV_OK;
  if (!d_base || !d_out) return LVKV_ERR_INVALID;
  KernelArgs a = blank_args();
  a.base = static_cast<const uint8_t*>(d_base);
  a.stride = stride;
  a.length = length;
  a.init = init;
  a.out_crc = d_out;
  a.mode = kModeCompute;
  a.mask = (flags & LVKV_FLAG_MASK) ? 1u : 0u;
  return run_batch(a, nblocks, static_cast<hipStream_t>(stream));
}

int lvkv_sst_verify_device(const void* d_file, const uint64_t* d_offsets,
                           const uint32_t* d_sizes, uint32_t* d_actual,
                           uint8_t* d_status, size_t nblocks, void* stream) {
  if (nblocks == 0) return LVKV_OK;
  if (!d_file || !d_offsets || !d_sizes || !d_actual || !d_status)
    return LVKV_ERR_INVALID;
  KernelArgs a = blank_args();
  a.base = static_cast<const uint8_t*>(d_file);
  a.offsets = d_offsets;
  a.lengths = d_sizes;
  a.out_crc = d_actual;
  a.out_status = d_status;
  a.mode = kModeSstVerify;
  return run_batch(a, nblocks, static_cast<hipStream_t>(stream));
}

int lvkv_sst_verify_table_device(const void* d_file, uint64_t file_size,
                                 uint64_t* d_offsets, uint32_t* d_sizes,
                                 uint32_t* d_actual, uint8_t* d_status, size_t capacity,
                                 const char* filter_policy, lvkv_sst_report* d_report,
                                 void* stream) {
  FilterKey fk;
  if (!d_file || !d_offsets || !d_sizes || !d_actual || !d_status || !d_report ||
      capacity == 0 || capacity > kMaxBlocksPerLaunch || !filter_key(filter_policy, &fk))
    return LVKV_ERR_INVALID;
  int rc = LVKV_OK;
  DeviceCtx* c = current_ctx(&rc);
  if (c == nullptr) return rc;
  KernelArgs a = ctx_args(*c);
  a.mode = kModeSstVerify;
  const hipError_t e = launch_sst_tables(
      static_cast<const uint8_t*>(d_file), nullptr, nullptr, file_size, 1, d_offsets, d_sizes,
      d_actual, d_status, static_cast<uint32_t>(capacity), d_report, fk, next_sst_generation(), a,
      c->d_tables + kZPowOffset, c->d_tables + kRowTabDwords + kLaneTabDwords, c->groups,
      sst_form(*c, file_size <= kFusedTableBytes), static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LVKV_OK : hip_fail(e);
}

int lvkv_sst_verify_tables_device(const void* d_file, const uint64_t* d_table_off,
                                  const uint64_t* d_table_size, size_t ntables,
                                  uint64_t* d_offsets, uint32_t* d_sizes, uint32_t* d_actual,
                                  uint8_t* d_status, size_t capacity, const char* filter_policy,
                                  lvkv_sst_report* d_reports, void* stream) {
  if (ntables == 0) return LVKV_OK;
  FilterKey fk;
  if (!d_file || !d_table_off || !d_table_size || !d_offsets || !d_sizes || !d_actual ||
      !d_status || !d_reports || capacity == 0 || capacity > kMaxBlocksPerLaunch ||
      ntables > (size_t{1} << 20) || !filter_key(filter_policy, &fk))
    return LVKV_ERR_INVALID;
  int rc = LVKV_OK;
  DeviceCtx* c = current_ctx(&rc);
  if (c == nullptr) return rc;
  KernelArgs a = ctx_args(*c);
  a.mode = kModeSstVerify;
  const hipError_t e = launch_sst_tables(
      static_cast<const uint8_t*>(d_file), d_table_off, d_table_size, 0,
      static_cast<uint32_t>(ntables), d_offsets, d_sizes, d_actual, d_status,
      static_cast<uint32_t>(capacity), d_reports, fk, next_sst_generation(), a,
      c->d_tables + kZPowOffset,
      c->d_tables + kRowTabDwords + kLaneTabDwords, c->groups,
      sst_form(*c, true, ntables), static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LVKV_OK : hip_fail(e);
}

int lvkv_log_verify_blocks_device(const void* d_file, uint64_t file_size,
                                  uint64_t* d_hdr_offsets, uint32_t* d_actual,
                                  uint8_t* d_rec_status, size_t capacity,
                                  uint8_t* d_block_status, uint32_t* d_block_drop,
                                  lvkv_log_report* d_report, void* stream) {
  if ((!d_file && file_size) || !d_hdr_offsets || !d_actual || !d_rec_status || !d_block_status ||
      !d_block_drop || !d_report || capacity == 0 || capacity > kMaxBlocksPerLaunch ||
      file_size > (uint64_t{1} << 46))
    return LVKV_ERR_INVALID;
  int rc = LVKV_OK;
  DeviceCtx* c = current_ctx(&rc);
  if (c == nullptr) return rc;
  const hipStream_t hs = static_cast<hipStream_t>(stream);
  void* scratch = nullptr;
  size_t slot = 0;
  hipError_t e = log_scratch_acquire(*c, hs, log_scratch_bytes(file_size, static_cast<uint32_t>(capacity), c->groups), &scratch, &slot);
  if (e == hipErrorStreamCaptureUnsupported) return LVKV_ERR_INVALID;
  if (e != hipSuccess) return hip_fail(e);
  e = launch_log_blocks(static_cast<const uint8_t*>(d_file), file_size, d_hdr_offsets, d_actual,
                        d_rec_status, static_cast<uint32_t>(capacity), d_block_status,
                        d_block_drop, d_report, c->d_tables + kZPowOffset,
                        c->d_tables + kRowTabDwords + kLaneTabDwords, c->groups, scratch, nullptr,
                        nullptr, hs);
  const hipError_t e2 = log_scratch_release(*c, slot, hs);
  if (e == hipSuccess) e = e2;
  return e == hipSuccess ? LVKV_OK : hip_fail(e);
}

int lvkv_log_read_device(const void* d_file, uint64_t file_size, uint64_t* d_hdr_offsets,
                         uint32_t* d_actual, uint8_t* d_rec_status, size_t capacity,
                         uint8_t* d_block_status, uint32_t* d_block_drop,
                         lvkv_log_report* d_report, lvkv_log_record* d_records,
                         size_t record_capacity, lvkv_log_corruption* d_reports,
                         size_t report_capacity, uint64_t initial_offset,
                         lvkv_log_read_report* d_read, void* stream) {
  if ((!d_file && file_size) || !d_hdr_offsets || !d_actual || !d_rec_status || !d_block_status ||
      !d_block_drop || !d_report || !d_read || (!d_records && record_capacity) ||
      (!d_reports && report_capacity) || capacity == 0 || capacity > kMaxBlocksPerLaunch ||
      record_capacity > kMaxBlocksPerLaunch || report_capacity > kMaxBlocksPerLaunch ||
      file_size > (uint64_t{1} << 46))
    return LVKV_ERR_INVALID;
  int rc = LVKV_OK;
  DeviceCtx* c = current_ctx(&rc);
  if (c == nullptr) return rc;
  const hipStream_t hs = static_cast<hipStream_t>(stream);
  // scratch: the verify's counters, the event stream (one u32 per candidate
  // record and per block) and the items' header offsets (u64 each), then the
  // logical layer's per-workgroup state
  const size_t nblocks = static_cast<size_t>((file_size + 32767) / 32768);
  const size_t ev_at =
      (log_scratch_bytes(file_size, static_cast<uint32_t>(capacity), c->groups) + 15) & ~size_t{15};
  const size_t off_at = (ev_at + (capacity + nblocks) * 4 + 15) & ~size_t{15};
  const size_t asm_at = (off_at + (capacity + nblocks) * 8 + 15) & ~size_t{15};
  void* scratch = nullptr;
  size_t slot = 0;
  hipError_t e = log_scratch_acquire(*c, hs, asm_at + log_asm_scratch_bytes(capacity + nblocks),
                                     &scratch, &slot);
  if (e == hipErrorStreamCaptureUnsupported) return LVKV_ERR_INVALID;
  if (e != hipSuccess) return hip_fail(e);
  uint8_t* sb = static_cast<uint8_t*>(scratch);
  uint32_t* events = reinterpret_cast<uint32_t*>(sb + ev_at);
  uint64_t* item_off = reinterpret_cast<uint64_t*>(sb + off_at);
  if (e == hipSuccess)
    e = launch_log_blocks(static_cast<const uint8_t*>(d_file), file_size, d_hdr_offsets,
                          d_actual, d_rec_status, static_cast<uint32_t>(capacity),
                          d_block_status, d_block_drop, d_report, c->d_tables + kZPowOffset,
                          c->d_tables + kRowTabDwords + kLaneTabDwords, c->groups, scratch,
                          events, item_off, hs);
  if (e == hipSuccess)
    e = launch_log_assemble(events, item_off, d_hdr_offsets, d_report, file_size,
                            static_cast<uint32_t>(capacity), initial_offset, d_records,
                            static_cast<uint32_t>(record_capacity), d_reports,
                            static_cast<uint32_t>(report_capacity), d_read, sb + asm_at, hs);
  const hipError_t e2 = log_scratch_release(*c, slot, hs);
  if (e == hipSuccess) e = e2;
  return e == hipSuccess ? LVKV_OK : hip_fail(e);
}

int lvkv_log_gather_device(const void* d_file, const uint64_t* d_hdr_offsets, size_t capacity,
                           const lvkv_log_report* d_report, const lvkv_log_record* d_records,
                           size_t record_capacity, const lvkv_log_read_report* d_read,
                           void* d_payload, uint64_t payload_capacity, uint64_t* d_record_pos,
                           void* stream) {
  if (!d_file || !d_hdr_offsets || !d_report || !d_read || (!d_records && record_capacity) ||
      (!d_payload && payload_capacity) || capacity == 0 || capacity > kMaxBlocksPerLaunch ||
      record_capacity > kMaxBlocksPerLaunch)
    return LVKV_ERR_INVALID;
  if (record_capacity == 0) return LVKV_OK;
  int rc = LVKV_OK;
  DeviceCtx* c = current_ctx(&rc);
  if (c == nullptr) return rc;
  const hipStream_t hs = static_cast<hipStream_t>(stream);
  void* scratch = nullptr;
  size_t slot = 0;
  // (the pool's buffers keep the verify's counters in bytes [0, 24), which
  // every call leaves at 0: the look-back slots go after them)
  hipError_t e =
      log_scratch_acquire(*c, hs, 32 + log_gather_scratch_bytes(capacity), &scratch, &slot);
  if (e == hipErrorStreamCaptureUnsupported) return LVKV_ERR_INVALID;
  if (e != hipSuccess) return hip_fail(e);
  // the look-back slots' tag: per call, 30 bits, never 0
  static std::atomic<uint32_t> tags{0};
  uint32_t tag;
  do {
    tag = (tags.fetch_add(1, std::memory_order_relaxed) + 1) & 0x3fffffffu;
  } while (tag == 0);
  e = launch_log_gather(static_cast<const uint8_t*>(d_file), d_hdr_offsets, capacity, d_report,
                        d_records, static_cast<uint32_t>(record_capacity), d_read,
                        static_cast<uint8_t*>(d_payload), payload_capacity, d_record_pos,
                        static_cast<uint8_t*>(scratch) + 32, tag, c->groups, hs);
  const hipError_t e2 = log_scratch_release(*c, slot, hs);
  if (e == hipSuccess) e = e2;
  return e == hipSuccess ? LVKV_OK : hip_fail(e);
}

int lvkv_sst_fill_trailers_device(void* d_file, const uint64_t* d_offsets,
                                  const uint32_t* d_sizes, uint32_t* d_crc, size_t nblocks,
                                  void* stream) {
  if (nblocks == 0) return LVKV_OK;
  if (!d_file || !d_offsets || !d_sizes) return LVKV_ERR_INVALID;
  KernelArgs a = blank_args();
  a.base = static_cast<const uint8_t*>(d_file);
  a.offsets = d_offsets;
  a.lengths = d_sizes;
  a.out_crc = d_crc;
  a.mode = kModeSstFill;
  return run_batch(a, nblocks, static_cast<hipStream_t>(stream));
}

int lvkv_log_fill_headers_device(void* d_file, const uint64_t* d_hdr_offsets, uint32_t* d_crc,
                                 size_t nrecords, void* stream) {
  if (nrecords == 0) return LVKV_OK;
  if (!d_file || !d_hdr_offsets) return LVKV_ERR_INVALID;
  KernelArgs a = blank_args();
  a.base = static_cast<const uint8_t*>(d_file);
  a.offsets = d_hdr_offsets;
  a.out_crc = d_crc;
  a.mode = kModeLogFill;
  return run_batch(a, nrecords, static_cast<hipStream_t>(stream));
}

int lvkv_log_verify_device(const void* d_file, const uint64_t* d_hdr_offsets,
                           uint32_t* d_actual, uint8_t* d_status,
                           size_t nrecords, void* stream) {
  if (nrecords == 0) return LVKV_OK;
  if (!d_file || !d_hdr_offsets || !d_actual || !d_status)
    return LVKV_ERR_INVALID;
  KernelArgs a = blank_args();
  a.base = static_cast<const uint8_t*>(d_file);
  a.offsets = d_hdr_offsets;
  a.out_crc = d_actual;
  a.out_status = d_status;
  a.mode = kModeLogVerify;
  return run_batch(a, nrecords, static_cast<hipStream_t>(stream));
}

size_t lvkv_snappy_max_compressed_length(size_t n) { return snappy_bound(n); }

int lvkv_snappy_compress_device(const void* d_src, const uint64_t* d_src_off,
                                const uint32_t* d_src_len, void* d_dst,
                                const uint64_t* d_dst_off, uint32_t* d_dst_len,
                                uint8_t* d_status, size_t nblocks, uint32_t max_len,
                                void* stream) {
  if (nblocks == 0) return LVKV_OK;
  if (!d_src || !d_src_off || !d_src_len || !d_dst || !d_dst_off || !d_dst_len || !d_status ||
      nblocks > kMaxBlocksPerLaunch)
    return LVKV_ERR_INVALID;
  int rc = LVKV_OK;
  if (current_ctx(&rc) == nullptr) return rc;
  const hipError_t e = launch_snappy_compress(
      static_cast<const uint8_t*>(d_src), d_src_off, d_src_len, static_cast<uint8_t*>(d_dst),
      d_dst_off, d_dst_len, d_status, static_cast<uint32_t>(nblocks), max_len, 0,
      static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LVKV_OK : hip_fail(e);
}

int lvkv_snappy_uncompressed_length_device(const void* d_src, const uint64_t* d_src_off,
                                           const uint32_t* d_src_len, uint32_t* d_ulen,
                                           uint8_t* d_status, size_t nblocks, void* stream) {
  if (nblocks == 0) return LVKV_OK;
  if (!d_src || !d_src_off || !d_src_len || !d_ulen || !d_status ||
      nblocks > kMaxBlocksPerLaunch)
    return LVKV_ERR_INVALID;
  int rc = LVKV_OK;
  if (current_ctx(&rc) == nullptr) return rc;
  const hipError_t e = launch_snappy_uncompress(
      static_cast<const uint8_t*>(d_src), d_src_off, d_src_len, nullptr, nullptr, nullptr,
      d_ulen, d_status, static_cast<uint32_t>(nblocks), 0, 0, nullptr,
      static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LVKV_OK : hip_fail(e);
}

int lvkv_snappy_uncompress_device(const void* d_src, const uint64_t* d_src_off,
                                  const uint32_t* d_src_len, void* d_dst,
                                  const uint64_t* d_dst_off, const uint32_t* d_dst_cap,
                                  uint32_t* d_out_len, uint8_t* d_status, size_t nblocks,
                                  uint32_t max_ulen, void* stream) {
  if (nblocks == 0) return LVKV_OK;
  if (!d_src || !d_src_off || !d_src_len || !d_dst || !d_dst_off || !d_dst_cap || !d_out_len ||
      !d_status || nblocks > kMaxBlocksPerLaunch || max_ulen > LVKV_SNAPPY_MAX_BLOCK)
    return LVKV_ERR_INVALID;
  int rc = LVKV_OK;
  if (current_ctx(&rc) == nullptr) return rc;
  const hipError_t e = launch_snappy_uncompress(
      static_cast<const uint8_t*>(d_src), d_src_off, d_src_len, static_cast<uint8_t*>(d_dst),
      d_dst_off, d_dst_cap, d_out_len, d_status, static_cast<uint32_t>(nblocks), max_ulen, 0,
      nullptr, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LVKV_OK : hip_fail(e);
}

size_t lvkv_sst_write_scratch_bytes(size_t nblocks, uint32_t max_len) {
  return nblocks * (snappy_write_stride(max_len) + 5);
}

size_t lvkv_zstd_compress_bound(size_t n) { return zstd_bound(n); }

int lvkv_zstd_compress_device(const void* d_src, const uint64_t* d_src_off,
                              const uint32_t* d_src_len, void* d_dst, const uint64_t* d_dst_off,
                              uint32_t* d_dst_len, uint8_t* d_status, size_t nblocks,
                              uint32_t max_len, int level, void* stream) {
  if (nblocks == 0) return LVKV_OK;
  if (!d_src || !d_src_off || !d_src_len || !d_dst || !d_dst_off || !d_dst_len || !d_status ||
      nblocks > kMaxBlocksPerLaunch || max_len > LVKV_ZSTD_COMPRESS_MAX_BLOCK)
    return LVKV_ERR_INVALID;
  int rc = LVKV_OK;
  if (current_ctx(&rc) == nullptr) return rc;
  const hipError_t e = launch_zstd_compress(
      static_cast<const uint8_t*>(d_src), d_src_off, d_src_len, static_cast<uint8_t*>(d_dst),
      d_dst_off, d_dst_len, d_status, static_cast<uint32_t>(nblocks), max_len, level, 0,
      static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LVKV_OK : hip_fail(e);
}

size_t lvkv_zstd_compress_big_scratch_bytes(uint32_t max_len) {
  return zstd_compress_big_scratch(max_len);
}

int lvkv_zstd_compress_big_device(const void* d_src, const uint64_t* d_src_off,
                                  const uint32_t* d_src_len, void* d_dst,
                                  const uint64_t* d_dst_off, uint32_t* d_dst_len,
                                  uint8_t* d_status, size_t nblocks, uint32_t max_len, int level,
                                  void* d_scratch, size_t scratch_bytes, void* stream) {
  if (nblocks == 0) return LVKV_OK;
  if (!d_src || !d_src_off || !d_src_len || !d_dst || !d_dst_off || !d_dst_len || !d_status ||
      nblocks > kMaxBlocksPerLaunch)
    return LVKV_ERR_INVALID;
  // (the lengths are on the device: a block can need the scratch whenever
  // max_len lets one past the first kernel's plan)
  const size_t need = zstd_compress_big_scratch(max_len);
  if (need != 0 && (!d_scratch || scratch_bytes < need)) return LVKV_ERR_INVALID;
  int rc = LVKV_OK;
  if (current_ctx(&rc) == nullptr) return rc;
  const hipError_t e = launch_zstd_compress_big(
      static_cast<const uint8_t*>(d_src), d_src_off, d_src_len, static_cast<uint8_t*>(d_dst),
      d_dst_off, d_dst_len, d_status, static_cast<uint32_t>(nblocks), max_len, level, 0,
      static_cast<uint8_t*>(d_scratch), static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LVKV_OK : hip_fail(e);
}

size_t lvkv_sst_write_scratch_bytes_v2(size_t nblocks, uint64_t total_raw_bytes, uint32_t max_len) {
  return sst_write_v2_bytes(nblocks, total_raw_bytes, max_len);
}

int lvkv_sst_write_blocks_status_device(const void* d_raw, const uint64_t* d_raw_off,
                                        const uint32_t* d_raw_len, size_t nblocks, int compression,
                                        int zstd_level, uint32_t max_len, void* d_scratch,
                                        void* d_file, uint64_t file_offset,
                                        uint64_t* d_handle_off, uint32_t* d_handle_size,
                                        uint8_t* d_type, uint64_t* d_end, size_t scratch_bytes,
                                        uint8_t* d_status, void* stream) {
  if (!d_end) return LVKV_ERR_INVALID;  // (nowhere to report even an empty batch)
  if (nblocks == 0) {  // before every other check: d_end = file_offset, by the layout kernel
    int rc = LVKV_OK;
    if (current_ctx(&rc) == nullptr) return rc;
    const hipError_t e = launch_sst_write_blocks(nullptr, nullptr, nullptr, 0, 0, 0, {}, nullptr,
                                                 file_offset, nullptr, nullptr, nullptr, d_end, 1,
                                                 nullptr, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? LVKV_OK : hip_fail(e);
  }
  if (compression < 0 || compression > 2) return LVKV_ERR_INVALID;
  if (compression == 2 && (zstd_level == 0 || zstd_level > 2)) return LVKV_ERR_INVALID;
  if (!d_raw || !d_raw_off || !d_raw_len || !d_file || !d_handle_off || !d_handle_size ||
      !d_type || !d_status || nblocks > kMaxBlocksPerLaunch)
    return LVKV_ERR_INVALID;
  if (compression != 0 &&
      (!d_scratch ||
       scratch_bytes < sst_write_v2_fixed(nblocks, compression == 2 ? max_len : 0u) + 16u))
    return LVKV_ERR_INVALID;
  int rc = LVKV_OK;
  if (current_ctx(&rc) == nullptr) return rc;
  const uint32_t n = static_cast<uint32_t>(nblocks);
  const SstWriteScratch scratch =
      compression == 0 ? SstWriteScratch{}
                       : sst_scratch_ragged(static_cast<uint8_t*>(d_scratch), scratch_bytes, n,
                                            compression == 2 ? max_len : 0u);
  const hipError_t e = launch_sst_write_blocks(
      static_cast<const uint8_t*>(d_raw), d_raw_off, d_raw_len, n, compression, max_len, scratch,
      static_cast<uint8_t*>(d_file), file_offset, d_handle_off, d_handle_size, d_type, d_end,
      zstd_level, d_status, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(e);
  return lvkv_sst_fill_trailers_device(d_file, d_handle_off, d_handle_size, nullptr, nblocks,
                                       stream);
}

size_t lvkv_sst_write_table_scratch_bytes(size_t nblocks, uint64_t total_raw_bytes,
                                          uint32_t max_len, uint32_t max_key_len,
                                          int filter_bits_per_key) {
  // alignment slack, the finisher's own part, the data blocks' ragged scratch
  return kScratchAlign + sst_finish_plan(nblocks, max_key_len, filter_bits_per_key).fixed +
         sst_write_v2_envelope(nblocks, total_raw_bytes, max_len);
}

uint64_t lvkv_sst_table_file_bound(size_t nblocks, uint64_t total_raw_bytes, uint32_t max_key_len,
                                   int filter_bits_per_key) {
  const uint64_t n = nblocks;
  const uint64_t data = total_raw_bytes + 5 * n;
  uint64_t filter = 0;
  if (filter_bits_per_key > 0) {
    // an entry takes 3 bytes or more; a filter of k keys max(64, k * bits)
    // bits rounded up and a probe count, at most one with keys a block; an
    // offset per 2 KiB of data and one; the array's offset, the base, the trailer
    const uint64_t keys = total_raw_bytes / 3;
    filter = keys * static_cast<uint64_t>(filter_bits_per_key) / 8 + 10 * n +
             4 * (data / 2048 + 1) + 5 + 5;
  }
  const uint64_t index = sst_finish_plan(nblocks, max_key_len, filter_bits_per_key).index_cap;
  return data + filter + (kSstMetaRoom + 5) + (index + 5) + 48;
}

// lvkv_sst_fill_trailers_device over the first min(n, *d_count) handles.
static int fill_trailers_counted(void* d_file, const uint64_t* d_offsets, const uint32_t* d_sizes,
                          size_t n, const uint32_t* d_count, hipStream_t stream) {
  KernelArgs a = blank_args();
  a.base = static_cast<const uint8_t*>(d_file);
  a.offsets = d_offsets;
  a.lengths = d_sizes;
  a.mode = kModeSstFill;
  a.count = d_count;
  return run_batch(a, n, stream);
}

int lvkv_sst_write_table_device(const void* d_raw, const uint64_t* d_raw_off,
                                const uint32_t* d_raw_len, size_t nblocks, int compression,
                                int zstd_level, uint32_t max_len, int key_format,
                                int filter_bits_per_key, uint32_t max_key_len, void* d_scratch,
                                size_t scratch_bytes, void* d_file, uint64_t file_capacity,
                                uint64_t* d_handle_off, uint32_t* d_handle_size, uint8_t* d_type,
                                uint8_t* d_status, lvkv_sst_table_report* d_report, void* stream) {
  if (!d_scratch || !d_file || !d_report) return LVKV_ERR_INVALID;
  if (nblocks != 0 && (!d_raw || !d_raw_off || !d_raw_len || !d_handle_off || !d_handle_size ||
                       !d_type || !d_status))
    return LVKV_ERR_INVALID;
  if (compression < 0 || compression > 2 || key_format < 0 || key_format > 1 ||
      filter_bits_per_key < 0 || max_key_len > (1u << 20))
    return LVKV_ERR_INVALID;
  if (compression == 2 && (zstd_level == 0 || zstd_level > 2)) return LVKV_ERR_INVALID;
  // (u32 block indices in every kernel; the index block's length is a u32)
  if (nblocks > kMaxBlocksPerLaunch ||
      uint64_t{nblocks} * (uint64_t{max_key_len} + 26) + 8 > 0xffffffffull)
    return LVKV_ERR_INVALID;
  if (scratch_bytes < lvkv_sst_write_table_scratch_bytes(nblocks, 0, max_len, max_key_len,
                                                         filter_bits_per_key))
    return LVKV_ERR_INVALID;
  int rc = LVKV_OK;
  if (current_ctx(&rc) == nullptr) return rc;
  const hipStream_t hs = static_cast<hipStream_t>(stream);
  const uint32_t n = static_cast<uint32_t>(nblocks);

  SstFinishArgs f{};
  f.raw = static_cast<const uint8_t*>(d_raw);
  f.raw_off = d_raw_off;
  f.raw_len = d_raw_len;
  f.nblocks = n;
  f.key_format = static_cast<uint32_t>(key_format);
  f.bits_per_key = static_cast<uint32_t>(filter_bits_per_key);
  // BloomFilterPolicy's constructor (util/bloom.cc:19-24)
  size_t k = static_cast<size_t>(filter_bits_per_key * 0.69);
  if (k < 1) k = 1;
  if (k > 30) k = 30;
  f.k = static_cast<uint32_t>(k);
  f.max_key_len = max_key_len;
  uint8_t* const scratch = static_cast<uint8_t*>(d_scratch);
  f.base = scratch_base(scratch);
  const SstFinishPlan plan = sst_finish_plan(nblocks, max_key_len, filter_bits_per_key);
  f.file = static_cast<uint8_t*>(d_file);
  f.cap = file_capacity;
  f.hoff = d_handle_off;
  f.hsize = d_handle_size;
  f.report = d_report;
  SstFinishCtl* ctl = reinterpret_cast<SstFinishCtl*>(f.base);

  hipError_t e = launch_sst_finish(f, 0, hs);
  if (e != hipSuccess) return hip_fail(e);
  // the data blocks, from file offset 0
  uint8_t* const data_scratch = f.base + plan.fixed;
  const SstWriteScratch ds =
      compression == 0 || n == 0
          ? SstWriteScratch{}
          : sst_scratch_ragged(data_scratch,
                               scratch_bytes - static_cast<size_t>(data_scratch - scratch), n,
                               compression == 2 ? max_len : 0u);
  const SstWriteDest data_dest{nullptr, file_capacity, &ctl->nfit_data};
  e = launch_sst_write_blocks(f.raw, d_raw_off, d_raw_len, n, compression, max_len, ds, f.file, 0,
                              d_handle_off, d_handle_size, d_type, &ctl->data_end, zstd_level,
                              d_status, hs, &data_dest);
  if (e != hipSuccess) return hip_fail(e);
  rc = fill_trailers_counted(d_file, d_handle_off, d_handle_size, n, &ctl->nfit_data, hs);
  if (rc != LVKV_OK) return rc;
  // the filter block in place, the metaindex and index contents in the scratch
  e = launch_sst_finish(f, 1, hs);
  if (e != hipSuccess) return hip_fail(e);
  // [metaindex, index] through the same writer, from the offset stage 1 left
  const SstWriteScratch ts =
      compression == 0
          ? SstWriteScratch{}
          : sst_scratch_ragged(f.base + plan.tail_scratch, plan.tail_scratch_bytes, 2,
                               compression == 2 ? plan.tail_max_len : 0u);
  const SstWriteDest tail_dest{&ctl->tail_base, file_capacity, &ctl->nfit_tail};
  e = launch_sst_write_blocks(f.base + plan.tail_raw, ctl->t_raw_off, ctl->t_raw_len, 2,
                              compression, plan.tail_max_len, ts, f.file, 0, ctl->t_hoff + 1,
                              ctl->t_hsize + 1, ctl->t_type, &ctl->tail_end, zstd_level,
                              ctl->t_status, hs, &tail_dest);
  if (e != hipSuccess) return hip_fail(e);
  e = launch_sst_finish(f, 2, hs);
  if (e != hipSuccess) return hip_fail(e);
  // the trailers of the filter block (where there is one) and of the two
  const size_t first = filter_bits_per_key != 0 ? 0 : 1;
  return fill_trailers_counted(d_file, ctl->t_hoff + first, ctl->t_hsize + first, 3 - first,
                               &ctl->tail_count, hs);
}

size_t lvkv_sst_build_blocks_scratch_bytes(size_t nentries, uint32_t restart_interval) {
  (void)restart_interval;  // (the arrays are per entry whatever the interval)
  return sst_build_scratch_bytes(nentries);
}

uint64_t lvkv_sst_build_blocks_raw_bound(size_t nentries, uint64_t total_key_bytes,
                                         uint64_t total_value_bytes, uint32_t restart_interval) {
  (void)restart_interval;  // (a block an entry: every entry a restart point)
  // three 5-byte varints, a restart, a block's count and its padding
  return total_key_bytes + total_value_bytes + uint64_t{nentries} * (15u + 4u + 4u + 15u);
}

int lvkv_sst_build_blocks_device(const void* d_keys, const uint64_t* d_key_off,
                                 const uint32_t* d_key_len, const void* d_vals,
                                 const uint64_t* d_val_off, const uint32_t* d_val_len,
                                 size_t nentries, uint32_t block_size, uint32_t restart_interval,
                                 int key_format, void* d_scratch, size_t scratch_bytes,
                                 void* d_raw, uint64_t raw_capacity, uint64_t* d_raw_off,
                                 uint32_t* d_raw_len, size_t max_blocks,
                                 lvkv_sst_build_report* d_report, void* stream) {
  SstBuildArgs a{};
  a.report = d_report;
  if (nentries == 0) {
    if (!d_report) return LVKV_OK;
    int rc = LVKV_OK;
    if (current_ctx(&rc) == nullptr) return rc;
    const hipError_t e = launch_sst_build(a, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? LVKV_OK : hip_fail(e);
  }
  if (!d_keys || !d_key_off || !d_key_len || !d_vals || !d_val_off || !d_val_len || !d_scratch ||
      !d_raw || !d_raw_off || !d_raw_len || !d_report)
    return LVKV_ERR_INVALID;
  if (restart_interval == 0 || key_format < 0 || key_format > 1 ||
      nentries >= (uint64_t{1} << 31) ||
      scratch_bytes < lvkv_sst_build_blocks_scratch_bytes(nentries, restart_interval))
    return LVKV_ERR_INVALID;
  int rc = LVKV_OK;
  if (current_ctx(&rc) == nullptr) return rc;
  a.keys = static_cast<const uint8_t*>(d_keys);
  a.key_off = d_key_off;
  a.key_len = d_key_len;
  a.vals = static_cast<const uint8_t*>(d_vals);
  a.val_off = d_val_off;
  a.val_len = d_val_len;
  a.n = static_cast<uint32_t>(nentries);
  a.block_size = block_size;
  a.restart_interval = restart_interval;
  a.key_format = static_cast<uint32_t>(key_format);
  a.scratch = static_cast<uint8_t*>(d_scratch);
  a.raw = static_cast<uint8_t*>(d_raw);
  a.raw_capacity = raw_capacity;
  a.raw_off = d_raw_off;
  a.raw_len = d_raw_len;
  a.max_blocks = max_blocks;
  const hipError_t e = launch_sst_build(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LVKV_OK : hip_fail(e);
}

size_t lvkv_sst_read_entries_scratch_bytes(size_t nblocks, uint64_t total_raw_bytes) {
  return sst_entries_scratch_bytes(nblocks, total_raw_bytes);
}

int lvkv_sst_read_entries_device(const void* d_raw, const uint64_t* d_raw_off,
                                 const uint32_t* d_raw_len, const uint8_t* d_skip, size_t nblocks,
                                 void* d_scratch, size_t scratch_bytes, void* d_keys,
                                 uint64_t key_capacity, uint64_t* d_key_off, uint32_t* d_key_len,
                                 uint64_t* d_val_off, uint32_t* d_val_len, size_t max_entries,
                                 uint64_t* d_block_first, uint8_t* d_block_status,
                                 lvkv_sst_entries_report* d_report, void* stream) {
  SstEntriesArgs a{};
  a.report = d_report;
  if (nblocks == 0) {
    if (!d_report) return LVKV_OK;
    int rc = LVKV_OK;
    if (current_ctx(&rc) == nullptr) return rc;
    const hipError_t e = launch_sst_entries(a, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? LVKV_OK : hip_fail(e);
  }
  if (!d_raw || !d_raw_off || !d_raw_len || !d_scratch || !d_keys || !d_key_off || !d_key_len ||
      !d_val_off || !d_val_len || !d_block_first || !d_block_status || !d_report)
    return LVKV_ERR_INVALID;
  if (nblocks >= (uint64_t{1} << 31) ||
      scratch_bytes < lvkv_sst_read_entries_scratch_bytes(nblocks, 0))
    return LVKV_ERR_INVALID;
  int rc = LVKV_OK;
  if (current_ctx(&rc) == nullptr) return rc;
  a.raw = static_cast<const uint8_t*>(d_raw);
  a.raw_off = d_raw_off;
  a.raw_len = d_raw_len;
  a.skip = d_skip;
  a.nblocks = static_cast<uint32_t>(nblocks);
  a.scratch = static_cast<uint8_t*>(d_scratch);
  a.scratch_bytes = scratch_bytes;
  a.keys = static_cast<uint8_t*>(d_keys);
  a.key_capacity = key_capacity;
  a.key_off = d_key_off;
  a.key_len = d_key_len;
  a.val_off = d_val_off;
  a.val_len = d_val_len;
  a.max_entries = max_entries;
  a.block_first = d_block_first;
  a.block_status = d_block_status;
  const hipError_t e = launch_sst_entries(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LVKV_OK : hip_fail(e);
}

size_t lvkv_sst_merge_entries_scratch_bytes(size_t nentries, uint32_t nruns) {
  (void)nruns;  // (the arrays are per entry whatever the runs are)
  return sst_merge_scratch_bytes(nentries);
}

int lvkv_sst_merge_entries_device(const void* d_keys, const uint64_t* d_key_off,
                                  const uint32_t* d_key_len, const void* d_vals,
                                  const uint64_t* d_val_off, const uint32_t* d_val_len,
                                  size_t nentries, const uint64_t* d_run_first, uint32_t nruns,
                                  int key_format, uint32_t flags, uint64_t smallest_snapshot,
                                  const void* d_deeper_keys, const uint64_t* d_deeper_off,
                                  const uint32_t* d_deeper_len, size_t n_deeper, void* d_scratch,
                                  size_t scratch_bytes, uint64_t* d_out_key_off,
                                  uint32_t* d_out_key_len, uint64_t* d_out_val_off,
                                  uint32_t* d_out_val_len, uint32_t* d_out_src, size_t max_out,
                                  uint32_t* d_dropped_src, lvkv_sst_merge_report* d_report,
                                  void* stream) {
  SstMergeArgs a{};
  a.report = d_report;
  if (nentries == 0) {
    if (!d_report) return LVKV_OK;
    int rc = LVKV_OK;
    if (current_ctx(&rc) == nullptr) return rc;
    const hipError_t e = launch_sst_merge(a, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? LVKV_OK : hip_fail(e);
  }
  if (!d_keys || !d_key_off || !d_key_len || !d_vals || !d_val_off || !d_val_len ||
      !d_run_first || !d_scratch || !d_out_key_off || !d_out_key_len || !d_out_val_off ||
      !d_out_val_len || !d_out_src || !d_report)
    return LVKV_ERR_INVALID;
  if (n_deeper != 0 && (!d_deeper_keys || !d_deeper_off || !d_deeper_len))
    return LVKV_ERR_INVALID;
  if (nruns < 1 || nruns > LVKV_MERGE_MAX_RUNS || key_format < 0 || key_format > 1 ||
      (flags & ~LVKV_MERGE_COMPACT) != 0 || ((flags & LVKV_MERGE_COMPACT) && key_format == 0) ||
      nentries >= (uint64_t{1} << 31) || n_deeper >= (uint64_t{1} << 31) ||
      scratch_bytes < lvkv_sst_merge_entries_scratch_bytes(nentries, nruns))
    return LVKV_ERR_INVALID;
  int rc = LVKV_OK;
  if (current_ctx(&rc) == nullptr) return rc;
  a.keys = static_cast<const uint8_t*>(d_keys);
  a.key_off = d_key_off;
  a.key_len = d_key_len;
  a.val_off = d_val_off;
  a.val_len = d_val_len;
  a.run_first = d_run_first;
  a.n = static_cast<uint32_t>(nentries);
  a.nruns = nruns;
  a.key_format = static_cast<uint32_t>(key_format);
  a.compact = (flags & LVKV_MERGE_COMPACT) ? 1u : 0u;
  a.smallest_snapshot = smallest_snapshot;
  a.deeper_keys = static_cast<const uint8_t*>(d_deeper_keys);
  a.deeper_off = d_deeper_off;
  a.deeper_len = d_deeper_len;
  a.n_deeper = static_cast<uint32_t>(n_deeper);
  a.scratch = static_cast<uint8_t*>(d_scratch);
  a.out_key_off = d_out_key_off;
  a.out_key_len = d_out_key_len;
  a.out_val_off = d_out_val_off;
  a.out_val_len = d_out_val_len;
  a.out_src = d_out_src;
  a.max_out = max_out;
  a.dropped_src = d_dropped_src;
  const hipError_t e = launch_sst_merge(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LVKV_OK : hip_fail(e);
}

size_t lvkv_sst_get_locate_scratch_bytes(uint32_t index_len, size_t nqueries) {
  return sst_get_locate_scratch_bytes(index_len, nqueries);
}

size_t lvkv_sst_get_seek_scratch_bytes(size_t nqueries) {
  return sst_get_seek_scratch_bytes(nqueries);
}

int lvkv_sst_get_locate_device(const void* d_index, uint32_t index_len, const void* d_filter,
                               uint32_t filter_len, const void* d_qkeys,
                               const uint64_t* d_qkey_off, const uint32_t* d_qkey_len,
                               size_t nqueries, int key_format, void* d_scratch,
                               size_t scratch_bytes, uint32_t* d_q_block,
                               uint64_t* d_q_handle_off, uint32_t* d_q_handle_size,
                               uint8_t* d_q_status, lvkv_sst_get_locate_report* d_report,
                               void* stream) {
  SstGetLocateArgs a{};
  a.report = d_report;
  if (nqueries == 0) {
    if (!d_report) return LVKV_OK;
    int rc = LVKV_OK;
    if (current_ctx(&rc) == nullptr) return rc;
    const hipError_t e = launch_sst_get_locate(a, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? LVKV_OK : hip_fail(e);
  }
  if (!d_index || !d_qkeys || !d_qkey_off || !d_qkey_len || !d_scratch || !d_q_block ||
      !d_q_handle_off || !d_q_handle_size || !d_q_status || !d_report)
    return LVKV_ERR_INVALID;
  if (nqueries >= (uint64_t{1} << 31) || key_format < 0 || key_format > 1 ||
      scratch_bytes < lvkv_sst_get_locate_scratch_bytes(index_len, nqueries))
    return LVKV_ERR_INVALID;
  int rc = LVKV_OK;
  if (current_ctx(&rc) == nullptr) return rc;
  a.index = static_cast<const uint8_t*>(d_index);
  a.index_len = index_len;
  a.filter = static_cast<const uint8_t*>(d_filter);
  a.filter_len = filter_len;
  a.qkeys = static_cast<const uint8_t*>(d_qkeys);
  a.qkey_off = d_qkey_off;
  a.qkey_len = d_qkey_len;
  a.n = static_cast<uint32_t>(nqueries);
  a.key_format = static_cast<uint32_t>(key_format);
  a.scratch = static_cast<uint8_t*>(d_scratch);
  a.q_block = d_q_block;
  a.q_handle_off = d_q_handle_off;
  a.q_handle_size = d_q_handle_size;
  a.q_status = d_q_status;
  const hipError_t e = launch_sst_get_locate(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LVKV_OK : hip_fail(e);
}

int lvkv_sst_get_seek_device(const void* d_raw, const uint64_t* d_raw_off,
                             const uint32_t* d_raw_len, const uint8_t* d_skip, size_t nblocks,
                             const void* d_qkeys, const uint64_t* d_qkey_off,
                             const uint32_t* d_qkey_len, const uint32_t* d_q_slot,
                             size_t nqueries, int key_format, void* d_scratch,
                             size_t scratch_bytes, uint32_t* d_hit_off,
                             uint64_t* d_val_off, uint32_t* d_val_len, uint64_t* d_tag,
                             uint8_t* d_state, lvkv_sst_get_seek_report* d_report, void* stream) {
  SstGetSeekArgs a{};
  a.report = d_report;
  if (nqueries == 0) {
    if (!d_report) return LVKV_OK;
    int rc = LVKV_OK;
    if (current_ctx(&rc) == nullptr) return rc;
    const hipError_t e = launch_sst_get_seek(a, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? LVKV_OK : hip_fail(e);
  }
  if (!d_raw || !d_raw_off || !d_raw_len || !d_qkeys || !d_qkey_off || !d_qkey_len || !d_q_slot ||
      !d_scratch || !d_hit_off || !d_val_off || !d_val_len || !d_tag || !d_state || !d_report)
    return LVKV_ERR_INVALID;
  if (nqueries >= (uint64_t{1} << 31) || nblocks >= (uint64_t{1} << 31) || key_format < 0 ||
      key_format > 1 || scratch_bytes < lvkv_sst_get_seek_scratch_bytes(nqueries))
    return LVKV_ERR_INVALID;
  int rc = LVKV_OK;
  if (current_ctx(&rc) == nullptr) return rc;
  a.raw = static_cast<const uint8_t*>(d_raw);
  a.raw_off = d_raw_off;
  a.raw_len = d_raw_len;
  a.skip = d_skip;
  a.nblocks = static_cast<uint32_t>(nblocks);
  a.qkeys = static_cast<const uint8_t*>(d_qkeys);
  a.qkey_off = d_qkey_off;
  a.qkey_len = d_qkey_len;
  a.q_slot = d_q_slot;
  a.n = static_cast<uint32_t>(nqueries);
  a.key_format = static_cast<uint32_t>(key_format);
  a.scratch = static_cast<uint8_t*>(d_scratch);
  a.hit_off = d_hit_off;
  a.val_off = d_val_off;
  a.val_len = d_val_len;
  a.tag = d_tag;
  a.state = d_state;
  const hipError_t e = launch_sst_get_seek(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LVKV_OK : hip_fail(e);
}

size_t lvkv_vtable_separate_scratch_bytes(size_t nentries) {
  return vtable_separate_scratch_bytes(nentries);
}

uint64_t lvkv_vtable_separate_vtb_bound(size_t nentries, uint64_t total_key_bytes,
                                        uint64_t total_value_bytes) {
  return total_key_bytes + total_value_bytes + uint64_t{nentries} * LVKV_VTABLE_RECORD_FRAMING;
}

uint64_t lvkv_vtable_separate_vals_bound(size_t nentries, uint64_t total_value_bytes) {
  return total_value_bytes + uint64_t{nentries} * LVKV_VTABLE_INDEX_MAX;
}

int lvkv_vtable_separate_device(const void* d_keys, const uint64_t* d_key_off,
                                const uint32_t* d_key_len, const void* d_vals,
                                const uint64_t* d_val_off, const uint32_t* d_val_len,
                                size_t nentries, uint64_t kv_sep_size, uint64_t file_number,
                                void* d_scratch, size_t scratch_bytes, void* d_vtb,
                                uint64_t vtb_capacity, void* d_out_vals,
                                uint64_t out_val_capacity, uint64_t* d_out_val_off,
                                uint32_t* d_out_val_len, uint64_t* d_rec_off,
                                uint64_t* d_rec_size, lvkv_vtable_separate_report* d_report,
                                void* stream) {
  VtableSeparateArgs a{};
  a.report = d_report;
  if (nentries == 0) {
    if (!d_report) return LVKV_OK;
    int rc = LVKV_OK;
    if (current_ctx(&rc) == nullptr) return rc;
    const hipError_t e = launch_vtable_separate(a, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? LVKV_OK : hip_fail(e);
  }
  if (!d_keys || !d_key_off || !d_key_len || !d_vals || !d_val_off || !d_val_len || !d_scratch ||
      !d_vtb || !d_out_vals || !d_out_val_off || !d_out_val_len || !d_report)
    return LVKV_ERR_INVALID;
  if (nentries >= (uint64_t{1} << 31) ||
      scratch_bytes < lvkv_vtable_separate_scratch_bytes(nentries))
    return LVKV_ERR_INVALID;
  int rc = LVKV_OK;
  if (current_ctx(&rc) == nullptr) return rc;
  a.keys = static_cast<const uint8_t*>(d_keys);
  a.key_off = d_key_off;
  a.key_len = d_key_len;
  a.vals = static_cast<const uint8_t*>(d_vals);
  a.val_off = d_val_off;
  a.val_len = d_val_len;
  a.n = static_cast<uint32_t>(nentries);
  a.kv_sep_size = kv_sep_size;
  a.file_number = file_number;
  a.scratch = static_cast<uint8_t*>(d_scratch);
  a.vtb = static_cast<uint8_t*>(d_vtb);
  a.vtb_capacity = vtb_capacity;
  a.out_vals = static_cast<uint8_t*>(d_out_vals);
  a.out_val_capacity = out_val_capacity;
  a.out_val_off = d_out_val_off;
  a.out_val_len = d_out_val_len;
  a.rec_off = d_rec_off;
  a.rec_size = d_rec_size;
  const hipError_t e = launch_vtable_separate(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LVKV_OK : hip_fail(e);
}

size_t lvkv_vtable_resolve_scratch_bytes(size_t nqueries) {
  return vtable_resolve_scratch_bytes(nqueries);
}

int lvkv_vtable_resolve_device(const void* d_vals, const uint64_t* d_val_off,
                               const uint32_t* d_val_len, const uint8_t* d_state,
                               size_t nqueries, const void* d_vtb, const uint64_t* d_file_off,
                               const uint64_t* d_file_size, const uint64_t* d_file_number,
                               size_t nfiles, void* d_scratch, size_t scratch_bytes,
                               uint8_t* d_status, uint8_t* d_out_src, uint64_t* d_out_off,
                               uint32_t* d_out_len, lvkv_vtable_resolve_report* d_report,
                               void* stream) {
  VtableResolveArgs a{};
  a.report = d_report;
  if (nqueries == 0) {
    if (!d_report) return LVKV_OK;
    int rc = LVKV_OK;
    if (current_ctx(&rc) == nullptr) return rc;
    const hipError_t e = launch_vtable_resolve(a, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? LVKV_OK : hip_fail(e);
  }
  if (!d_vals || !d_val_off || !d_val_len || !d_scratch || !d_status || !d_out_src ||
      !d_out_off || !d_out_len || !d_report)
    return LVKV_ERR_INVALID;
  if (nfiles != 0 && (!d_vtb || !d_file_off || !d_file_size || !d_file_number))
    return LVKV_ERR_INVALID;
  if (nqueries >= (uint64_t{1} << 31) || nfiles >= (uint64_t{1} << 31) ||
      scratch_bytes < lvkv_vtable_resolve_scratch_bytes(nqueries))
    return LVKV_ERR_INVALID;
  int rc = LVKV_OK;
  if (current_ctx(&rc) == nullptr) return rc;
  a.vals = static_cast<const uint8_t*>(d_vals);
  a.val_off = d_val_off;
  a.val_len = d_val_len;
  a.state = d_state;
  a.n = static_cast<uint32_t>(nqueries);
  a.vtb = static_cast<const uint8_t*>(d_vtb);
  a.file_off = d_file_off;
  a.file_size = d_file_size;
  a.file_number = d_file_number;
  a.nfiles = static_cast<uint32_t>(nfiles);
  a.scratch = static_cast<uint8_t*>(d_scratch);
  a.status = d_status;
  a.out_src = d_out_src;
  a.out_off = d_out_off;
  a.out_len = d_out_len;
  const hipError_t e = launch_vtable_resolve(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LVKV_OK : hip_fail(e);
}

size_t lvkv_vtable_gather_scratch_bytes(size_t nqueries) {
  return vtable_gather_scratch_bytes(nqueries);
}

int lvkv_vtable_gather_device(const void* d_vals, const void* d_vtb, const uint8_t* d_status,
                              const uint8_t* d_out_src, const uint64_t* d_out_off,
                              const uint32_t* d_out_len, size_t nqueries, void* d_scratch,
                              size_t scratch_bytes, void* d_dst, uint64_t dst_capacity,
                              uint64_t* d_dst_off, lvkv_vtable_gather_report* d_report,
                              void* stream) {
  VtableGatherArgs a{};
  a.report = d_report;
  if (nqueries == 0) {
    if (!d_report) return LVKV_OK;
    int rc = LVKV_OK;
    if (current_ctx(&rc) == nullptr) return rc;
    const hipError_t e = launch_vtable_gather(a, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? LVKV_OK : hip_fail(e);
  }
  if (!d_vals || !d_vtb || !d_status || !d_out_src || !d_out_off || !d_out_len || !d_scratch ||
      !d_dst || !d_dst_off || !d_report)
    return LVKV_ERR_INVALID;
  if (nqueries >= (uint64_t{1} << 31) ||
      scratch_bytes < lvkv_vtable_gather_scratch_bytes(nqueries))
    return LVKV_ERR_INVALID;
  int rc = LVKV_OK;
  if (current_ctx(&rc) == nullptr) return rc;
  a.vals = static_cast<const uint8_t*>(d_vals);
  a.vtb = static_cast<const uint8_t*>(d_vtb);
  a.status = d_status;
  a.out_src = d_out_src;
  a.out_off = d_out_off;
  a.out_len = d_out_len;
  a.n = static_cast<uint32_t>(nqueries);
  a.scratch = static_cast<uint8_t*>(d_scratch);
  a.dst = static_cast<uint8_t*>(d_dst);
  a.dst_capacity = dst_capacity;
  a.dst_off = d_dst_off;
  const hipError_t e = launch_vtable_gather(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LVKV_OK : hip_fail(e);
}

size_t lvkv_memtable_scratch_bytes(size_t nbatches, size_t max_entries) {
  return memtable_scratch_bytes(nbatches, max_entries);
}

int lvkv_debug_set_memtable_tile(int pairs) {
  return memtable_set_tile(pairs) ? LVKV_OK : LVKV_ERR_INVALID;
}

int lvkv_memtable_from_batches_device(const void* d_payload, const uint64_t* d_batch_off,
                                      const uint64_t* d_batch_len, size_t nbatches,
                                      uint64_t max_sequence_in, uint32_t flags, void* d_scratch,
                                      size_t scratch_bytes, void* d_keys, uint64_t key_capacity,
                                      uint64_t* d_key_off, uint32_t* d_key_len,
                                      uint64_t* d_val_off, uint32_t* d_val_len, uint32_t* d_src,
                                      size_t max_entries, uint8_t* d_batch_status,
                                      uint32_t* d_batch_entries, lvkv_memtable_report* d_report,
                                      void* stream) {
  MemtableArgs a{};
  a.report = d_report;
  a.max_sequence_in = max_sequence_in;
  if (nbatches == 0) {
    if (!d_report) return LVKV_OK;
    int rc = LVKV_OK;
    if (current_ctx(&rc) == nullptr) return rc;
    const hipError_t e = launch_memtable(a, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? LVKV_OK : hip_fail(e);
  }
  if (!d_payload || !d_batch_off || !d_batch_len || !d_scratch || !d_keys || !d_key_off ||
      !d_key_len || !d_val_off || !d_val_len || !d_src || !d_report)
    return LVKV_ERR_INVALID;
  if (nbatches >= (uint64_t{1} << 31) || max_entries >= (uint64_t{1} << 31) ||
      scratch_bytes < lvkv_memtable_scratch_bytes(nbatches, max_entries))
    return LVKV_ERR_INVALID;
  int rc = LVKV_OK;
  if (current_ctx(&rc) == nullptr) return rc;
  a.payload = static_cast<const uint8_t*>(d_payload);
  a.batch_off = d_batch_off;
  a.batch_len = d_batch_len;
  a.nbatches = static_cast<uint32_t>(nbatches);
  a.flags = flags;
  a.scratch = static_cast<uint8_t*>(d_scratch);
  a.keys = static_cast<uint8_t*>(d_keys);
  a.key_capacity = key_capacity;
  a.key_off = d_key_off;
  a.key_len = d_key_len;
  a.val_off = d_val_off;
  a.val_len = d_val_len;
  a.src = d_src;
  a.max_entries = static_cast<uint32_t>(max_entries);
  a.batch_status = d_batch_status;
  a.batch_entries = d_batch_entries;
  const hipError_t e = launch_memtable(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LVKV_OK : hip_fail(e);
}

size_t lvkv_sst_scan_entries_scratch_bytes(size_t nentries, size_t nqueries) {
  return sst_scan_scratch_bytes(nentries, nqueries);
}

int lvkv_sst_scan_entries_device(const void* d_keys, const uint64_t* d_key_off,
                                 const uint32_t* d_key_len, const uint64_t* d_val_off,
                                 const uint32_t* d_val_len, size_t nentries, uint64_t snapshot,
                                 const void* d_qkeys, const uint64_t* d_start_off,
                                 const uint32_t* d_start_len, const uint64_t* d_limit_off,
                                 const uint32_t* d_limit_len, const uint32_t* d_q_max,
                                 size_t nqueries, void* d_scratch, size_t scratch_bytes,
                                 uint64_t* d_out_key_off, uint32_t* d_out_key_len,
                                 uint64_t* d_out_val_off, uint32_t* d_out_val_len,
                                 uint32_t* d_out_src, size_t max_out, uint32_t* d_q_first,
                                 uint32_t* d_q_count, uint8_t* d_q_status,
                                 lvkv_sst_scan_report* d_report, void* stream) {
  SstScanArgs a{};
  a.report = d_report;
  if (nentries == 0) {
    if (!d_report) return LVKV_OK;
    int rc = LVKV_OK;
    if (current_ctx(&rc) == nullptr) return rc;
    const hipError_t e = launch_sst_scan(a, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? LVKV_OK : hip_fail(e);
  }
  if (!d_keys || !d_key_off || !d_key_len || !d_val_off || !d_val_len || !d_scratch ||
      !d_out_key_off || !d_out_key_len || !d_out_val_off || !d_out_val_len || !d_out_src ||
      !d_report)
    return LVKV_ERR_INVALID;
  if (nqueries != 0 && (!d_qkeys || !d_start_off || !d_start_len || !d_limit_off ||
                        !d_limit_len || !d_q_first || !d_q_count || !d_q_status))
    return LVKV_ERR_INVALID;
  if (snapshot > (uint64_t{1} << 56) - 1 || nentries >= (uint64_t{1} << 31) ||
      nqueries >= (uint64_t{1} << 31) ||
      scratch_bytes < lvkv_sst_scan_entries_scratch_bytes(nentries, nqueries))
    return LVKV_ERR_INVALID;
  int rc = LVKV_OK;
  if (current_ctx(&rc) == nullptr) return rc;
  a.keys = static_cast<const uint8_t*>(d_keys);
  a.key_off = d_key_off;
  a.key_len = d_key_len;
  a.val_off = d_val_off;
  a.val_len = d_val_len;
  a.n = static_cast<uint32_t>(nentries);
  a.snapshot = snapshot;
  a.qkeys = static_cast<const uint8_t*>(d_qkeys);
  a.start_off = d_start_off;
  a.start_len = d_start_len;
  a.limit_off = d_limit_off;
  a.limit_len = d_limit_len;
  a.q_max = d_q_max;
  a.nq = static_cast<uint32_t>(nqueries);
  a.scratch = static_cast<uint8_t*>(d_scratch);
  a.out_key_off = d_out_key_off;
  a.out_key_len = d_out_key_len;
  a.out_val_off = d_out_val_off;
  a.out_val_len = d_out_val_len;
  a.out_src = d_out_src;
  a.max_out = max_out;
  a.q_first = d_q_first;
  a.q_count = d_q_count;
  a.q_status = d_q_status;
  const hipError_t e = launch_sst_scan(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LVKV_OK : hip_fail(e);
}

int lvkv_sst_write_blocks_device(const void* d_raw, const uint64_t* d_raw_off,
                                 const uint32_t* d_raw_len, size_t nblocks, int compression,
                                 uint32_t max_len, void* d_scratch, void* d_file,
                                 uint64_t file_offset, uint64_t* d_handle_off,
                                 uint32_t* d_handle_size, uint8_t* d_type, uint64_t* d_end,
                                 void* stream) {
  return lvkv_sst_write_blocks_level_device(d_raw, d_raw_off, d_raw_len, nblocks, compression, 1,
                                            max_len, d_scratch, d_file, file_offset, d_handle_off,
                                            d_handle_size, d_type, d_end, stream);
}

int lvkv_sst_write_blocks_level_device(const void* d_raw, const uint64_t* d_raw_off,
                                       const uint32_t* d_raw_len, size_t nblocks, int compression,
                                       int zstd_level, uint32_t max_len, void* d_scratch,
                                       void* d_file, uint64_t file_offset, uint64_t* d_handle_off,
                                       uint32_t* d_handle_size, uint8_t* d_type, uint64_t* d_end,
                                       void* stream) {
  if (!d_end || compression < 0 || compression > 2) return LVKV_ERR_INVALID;
  // kZstdCompression on the device: the ZSTD_fast levels (<= 2; 0 means 3)
  // and blocks the compressor's LDS plan holds
  if (compression == 2 &&
      (zstd_level == 0 || zstd_level > 2 || max_len > LVKV_ZSTD_COMPRESS_MAX_BLOCK))
    return LVKV_ERR_INVALID;
  if (nblocks == 0) {  // d_end = file_offset, by the layout kernel (no host pointer kept)
    int rc = LVKV_OK;
    if (current_ctx(&rc) == nullptr) return rc;
    const hipError_t e = launch_sst_write_blocks(nullptr, nullptr, nullptr, 0, compression, 0, {},
                                                 nullptr, file_offset, nullptr, nullptr, nullptr,
                                                 d_end, zstd_level, nullptr,
                                                 static_cast<hipStream_t>(stream));
    return e == hipSuccess ? LVKV_OK : hip_fail(e);
  }
  if (!d_raw || !d_raw_off || !d_raw_len || !d_file || !d_handle_off || !d_handle_size ||
      !d_type || (compression != 0 && !d_scratch) || nblocks > kMaxBlocksPerLaunch)
    return LVKV_ERR_INVALID;
  int rc = LVKV_OK;
  if (current_ctx(&rc) == nullptr) return rc;
  const hipStream_t hs = static_cast<hipStream_t>(stream);
  const uint32_t n = static_cast<uint32_t>(nblocks);
  const SstWriteScratch scratch =
      compression == 0
          ? SstWriteScratch{}
          : sst_scratch_strided(static_cast<uint8_t*>(d_scratch), d_raw_len, n, max_len);
  hipError_t e = launch_sst_write_blocks(
      static_cast<const uint8_t*>(d_raw), d_raw_off, d_raw_len, n, compression, max_len, scratch,
      static_cast<uint8_t*>(d_file), file_offset, d_handle_off, d_handle_size, d_type, d_end,
      zstd_level, nullptr, hs);
  if (e != hipSuccess) return hip_fail(e);
  // the trailers: Mask(CRC32C(contents + type)) by the batch CRC kernel
  return lvkv_sst_fill_trailers_device(d_file, d_handle_off, d_handle_size, nullptr, nblocks,
                                       stream);
}

int lvkv_sst_read_blocks_device(const void* d_file, const uint64_t* d_handle_off,
                                const uint32_t* d_handle_size, size_t nblocks, int verify,
                                void* d_out, const uint64_t* d_out_off, const uint32_t* d_out_cap,
                                uint32_t* d_out_len, uint8_t* d_status, uint32_t max_ulen,
                                void* stream) {
  if (nblocks == 0) return LVKV_OK;
  if (!d_file || !d_handle_off || !d_handle_size || !d_out || !d_out_off || !d_out_cap ||
      !d_out_len || !d_status || nblocks > kMaxBlocksPerLaunch ||
      max_ulen > LVKV_SNAPPY_MAX_BLOCK)
    return LVKV_ERR_INVALID;
  int rc = LVKV_OK;
  if (current_ctx(&rc) == nullptr) return rc;
  if (verify) {  // the verdicts land in d_status (the CRCs in d_out_len) first
    rc = lvkv_sst_verify_device(d_file, d_handle_off, d_handle_size, d_out_len, d_status,
                                nblocks, stream);
    if (rc != LVKV_OK) return rc;
  }
  const hipError_t e = launch_sst_read_blocks(
      static_cast<const uint8_t*>(d_file), d_handle_off, d_handle_size,
      static_cast<uint32_t>(nblocks), static_cast<uint8_t*>(d_out), d_out_off, d_out_cap,
      d_out_len, d_status, verify ? d_status : nullptr, max_ulen,
      static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LVKV_OK : hip_fail(e);
}

int lvkv_zstd_uncompressed_length_device(const void* d_src, const uint64_t* d_src_off,
                                         const uint32_t* d_src_len, uint32_t* d_ulen,
                                         uint8_t* d_status, size_t nblocks, void* stream) {
  if (nblocks == 0) return LVKV_OK;
  if (!d_src || !d_src_off || !d_src_len || !d_ulen || !d_status ||
      nblocks > kMaxBlocksPerLaunch)
    return LVKV_ERR_INVALID;
  int rc = LVKV_OK;
  if (current_ctx(&rc) == nullptr) return rc;
  const hipError_t e = launch_zstd_uncompress(
      static_cast<const uint8_t*>(d_src), d_src_off, d_src_len, nullptr, nullptr, nullptr,
      d_ulen, d_status, nullptr, static_cast<uint32_t>(nblocks), 0, 0, nullptr,
      static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LVKV_OK : hip_fail(e);
}

static int zstd_uncompress(const void* d_src, const uint64_t* d_src_off, const uint32_t* d_src_len,
                    void* d_dst, const uint64_t* d_dst_off, const uint32_t* d_dst_cap,
                    uint32_t* d_out_len, uint8_t* d_status, uint32_t* d_detail, size_t nblocks,
                    uint32_t max_ulen, void* stream) {
  if (nblocks == 0) return LVKV_OK;
  if (!d_src || !d_src_off || !d_src_len || !d_dst || !d_dst_off || !d_dst_cap || !d_out_len ||
      !d_status || nblocks > kMaxBlocksPerLaunch || max_ulen > LVKV_SNAPPY_MAX_BLOCK)
    return LVKV_ERR_INVALID;
  int rc = LVKV_OK;
  if (current_ctx(&rc) == nullptr) return rc;
  const hipError_t e = launch_zstd_uncompress(
      static_cast<const uint8_t*>(d_src), d_src_off, d_src_len, static_cast<uint8_t*>(d_dst),
      d_dst_off, d_dst_cap, d_out_len, d_status, d_detail, static_cast<uint32_t>(nblocks),
      max_ulen, 0, nullptr, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LVKV_OK : hip_fail(e);
}

int lvkv_zstd_uncompress_device(const void* d_src, const uint64_t* d_src_off,
                                const uint32_t* d_src_len, void* d_dst, const uint64_t* d_dst_off,
                                const uint32_t* d_dst_cap, uint32_t* d_out_len, uint8_t* d_status,
                                size_t nblocks, uint32_t max_ulen, void* stream) {
  return zstd_uncompress(d_src, d_src_off, d_src_len, d_dst, d_dst_off, d_dst_cap, d_out_len,
                         d_status, nullptr, nblocks, max_ulen, stream);
}

int lvkv_debug_zstd_uncompress_device(const void* d_src, const uint64_t* d_src_off,
                                      const uint32_t* d_src_len, void* d_dst,
                                      const uint64_t* d_dst_off, const uint32_t* d_dst_cap,
                                      uint32_t* d_out_len, uint8_t* d_status, uint32_t* d_detail,
                                      size_t nblocks, uint32_t max_ulen, void* stream) {
  return zstd_uncompress(d_src, d_src_off, d_src_len, d_dst, d_dst_off, d_dst_cap, d_out_len,
                         d_status, d_detail, nblocks, max_ulen, stream);
}

int lvkv_crc32c_batch_host(const void* h_base, const uint64_t* offsets,
                           const uint32_t* lengths, const uint32_t* init_arr,
                           uint32_t init, uint32_t* h_out, size_t nblocks,
                           uint32_t flags) {
  if (nblocks == 0) return LVKV_OK;
  if (!h_base || !offsets || !lengths || !h_out) return LVKV_ERR_INVALID;
  int rc = LVKV_OK;
  DeviceCtx* c = current_ctx(&rc);
  if (c == nullptr) return rc;
  std::lock_guard<std::mutex> lock(c->host_mu);
  size_t biggest = 0;
  for (size_t i = 0; i < nblocks; ++i)
    biggest = std::max<size_t>(biggest, lengths[i]);
  rc = ensure_stages(*c, biggest + 8);
  if (rc != LVKV_OK) return rc;
  // Every return leaves both stages idle: on an error the stage still in
  // flight is waited for and dropped, so no later call copies its results.
  struct StageGuard {
    DeviceCtx* c;
    ~StageGuard() {
      for (Stage& s : c->stage) {
        if (s.busy) (void)hipStreamSynchronize(s.stream);
        s.busy = false;
      }
    }
  } guard{c};
  const uint8_t* src = static_cast<const uint8_t*>(h_base);

  size_t next = 0;
  int k = 0;
  std::vector<uint64_t> src_off;
  while (next < nblocks) {
    Stage& s = c->stage[k];
    rc = drain_stage(s, h_out);
    if (rc != LVKV_OK) return rc;
    // Pack blocks so each one ENDS on a 4-byte boundary (the kernel's
    // aligned fast path), as many as fit.
    size_t n = 0, cursor = 0;
    src_off.clear();
    while (next + n < nblocks && n < kStageBlocks) {
      const size_t len = lengths[next + n];
      const size_t end = (cursor + len + 3) & ~size_t{3};
      if (end > s.cap) break;
      s.h_off[n] = end - len;
      s.h_len[n] = static_cast<uint32_t>(len);
      s.h_init[n] = init_arr ? init_arr[next + n] : init;
      src_off.push_back(offsets[next + n]);
      cursor = end;
      ++n;
    }
    pack_parallel(s.h_data, src, src_off.data(), s.h_len, s.h_off, n, cursor);
    hipError_t e;
    if ((e = hipMemcpyAsync(s.d_data, s.h_data, cursor, hipMemcpyHostToDevice,
                            s.stream)) != hipSuccess ||
        (e = hipMemcpyAsync(s.d_off, s.h_off, n * 8, hipMemcpyHostToDevice,
                            s.stream)) != hipSuccess ||
        (e = hipMemcpyAsync(s.d_len, s.h_len, n * 4, hipMemcpyHostToDevice,
                            s.stream)) != hipSuccess ||
        (e = hipMemcpyAsync(s.d_init, s.h_init, n * 4, hipMemcpyHostToDevice,
                            s.stream)) != hipSuccess)
      return hip_fail(e);
    rc = lvkv_crc32c_batch_device(s.d_data, s.d_off, s.d_len, s.d_init, 0,
                                  s.d_out, n, flags, s.stream);
    if (rc != LVKV_OK) return rc;
    if ((e = hipMemcpyAsync(s.h_out, s.d_out, n * 4, hipMemcpyDeviceToHost,
                            s.stream)) != hipSuccess ||
        (e = hipEventRecord(s.done, s.stream)) != hipSuccess)
      return hip_fail(e);
    s.first = next;
    s.count = n;
    s.busy = true;
    next += n;
    k ^= 1;
  }
  for (Stage& s : c->stage) {
    rc = drain_stage(s, h_out);
    if (rc != LVKV_OK) return rc;
  }
  return LVKV_OK;
}

const char* lvkv_strerror(int code) {
  switch (code) {
    case LVKV_OK:
      return "ok";
    case LVKV_ERR_INVALID:
      return "invalid argument";
    case LVKV_ERR_NO_DEVICE:
      return "no HIP device available (the batch API has no CPU fallback)";
    case LVKV_ERR_HIP:
      return "HIP runtime error";
    case LVKV_ERR_RANGE:
      return "block too large";
    default:
      return "unknown error";
  }
}

int lvkv_last_hip_error(void) { return t_last_hip_error; }

const char* lvkv_cpu_impl(void) { return cpu_crc32c_impl_name(); }

#ifdef LVKV_PROBE_BUILD
// Probe entry points (tools/probe/liblvkv_probe.so only).
void lvkv_debug_log_stamps(uint64_t* d_stamps) { g_log_stamps = d_stamps; }
void lvkv_debug_asm_stamps(uint64_t* d_stamps) { g_asm_stamps = d_stamps; }
void lvkv_debug_sst_stamps(uint64_t* d_stamps) { g_sst_stamps = d_stamps; }
void lvkv_debug_log_knobs(uint32_t knobs) { g_log_knobs = knobs; }
void lvkv_debug_zstd_stamps(uint64_t* d_stamps) { g_zstd_stamps = d_stamps; }
void lvkv_debug_zstdc_stamps(uint64_t* d_stamps) { g_zstdc_stamps = d_stamps; }
static uint64_t* g_debug_stamps = nullptr;

void lvkv_debug_set_stamps(uint64_t* d_stamps) { g_debug_stamps = d_stamps; }

int lvkv_debug_uniform_variant(int variant, int groups, const void* d_base,
                               uint64_t stride, uint32_t length,
                               uint32_t* d_out, size_t nblocks, void* stream) {
  if (nblocks == 0) return LVKV_OK;
  if (!d_base || !d_out || nblocks > kMaxBlocksPerLaunch) return LVKV_ERR_INVALID;
  int rc = LVKV_OK;
  DeviceCtx* c = current_ctx(&rc);
  if (c == nullptr) return rc;
  KernelArgs a = blank_args();
  a.base = static_cast<const uint8_t*>(d_base);
  a.stride = stride;
  a.length = length;
  a.out_crc = d_out;
  a.nblocks = static_cast<uint32_t>(nblocks);
  a.row_tab = c->d_tables;
  a.lane_tab = c->d_tables + kRowTabDwords;
  a.stamps = g_debug_stamps;
  if ((variant & 64) && g_debug_stamps == nullptr) return LVKV_ERR_INVALID;
  const int g = groups > 0 ? groups : c->groups;
  hipError_t e;
  if (variant & 256) {
    if (length < 4 || (stride % 4) != 0 ||
        ((reinterpret_cast<uintptr_t>(d_base) + length) % 4) != 0)
      return LVKV_ERR_INVALID;
    if (variant & 2048) {
      // compact-LDS kernel (crc32c_compact.hip), cfg in bits 16..22
      const int cfg = (variant >> 16) & 0x7f;
      const int gg = groups > 0 ? groups : c->groups * compact_occupancy(cfg);
      if (length > kRowsPerChunk * kRowBytes ||
          nblocks > static_cast<size_t>(gg) * compact_capacity(cfg))
        return LVKV_ERR_INVALID;
      e = launch_crc32c_compact(uniform_args(*c, a), cfg, gg, static_cast<hipStream_t>(stream));
    } else if (variant & 512) {
      if (length > kRowsPerChunk * kRowBytes ||
          nblocks > 3 * static_cast<size_t>(g) * kWavesPerGroup)
        return LVKV_ERR_INVALID;
      // debug bit 1024 -> kernel bit 256 (kSmallHalfA), 16384 -> 4096 (memory-only probe)
      // variant >= 1 << 16: kernel bits given directly in bits 16..30
      const int sv = variant >= (1 << 16)
                         ? (variant >> 16) | (variant & 64)
                         : (variant & 255) | ((variant & 1024) >> 2) | ((variant & 16384) >> 2);
      e = launch_crc32c_uniform_small(uniform_args(*c, a), sv, g,
                                      static_cast<hipStream_t>(stream));
    } else {
      e = launch_crc32c_uniform(uniform_args(*c, a), variant & 255, g,
                                static_cast<hipStream_t>(stream));
    }
  } else {
    e = launch_crc32c_probe(a, variant, g, static_cast<hipStream_t>(stream));
  }
  return e == hipSuccess ? LVKV_OK : hip_fail(e);
}

int lvkv_debug_read_bw(const void* d_data, uint64_t bytes, uint32_t* d_scratch,
                       int groups, void* stream) {
  if (!d_data || !d_scratch || (bytes & 15u)) return LVKV_ERR_INVALID;
  int rc = LVKV_OK;
  DeviceCtx* c = current_ctx(&rc);
  if (c == nullptr) return rc;
  const int g = groups != 0 ? groups : 8 * c->groups;
  hipError_t e = launch_read_bw(d_data, bytes, d_scratch, g,
                                static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LVKV_OK : hip_fail(e);
}

#endif  // LVKV_PROBE_BUILD

// -1: crc32c_kernel.hip's persistent kernel for general-layout batches;
// 0..31: crc32c_ragged.hip cfgs (launch_crc32c_ragged). Timing only.
int lvkv_debug_set_general_kernel(int k) {
  if (k < -1 || k > 31) return LVKV_ERR_INVALID;
  int rc = LVKV_OK;
  DeviceCtx* c = current_ctx(&rc);
  if (c == nullptr) return rc;
  c->general_cfg.store(k, std::memory_order_relaxed);
  return LVKV_OK;
}

// The ragged cfg used for WAL records (8, 16, 24: small-record shapes).
int lvkv_debug_set_vtable_copy_rows(int rows) {
  return vtable_set_copy_rows(rows) ? LVKV_OK : LVKV_ERR_INVALID;
}

int lvkv_debug_set_log_kernel(int k) {
  if (k < 0 || k > 31) return LVKV_ERR_INVALID;
  int rc = LVKV_OK;
  DeviceCtx* c = current_ctx(&rc);
  if (c == nullptr) return rc;
  c->log_cfg.store(k, std::memory_order_relaxed);
  return LVKV_OK;
}

// Whole-SSTable verify form: 0 by size (default), 1 always the fused launch,
// 2 always the two launches, 3 the speculative launch where it applies.
// Timing and tests.
int lvkv_debug_set_sst_form(int form) {
  if (form < 0 || form > 3) return LVKV_ERR_INVALID;
  int rc = LVKV_OK;
  DeviceCtx* c = current_ctx(&rc);
  if (c == nullptr) return rc;
  c->sst_form.store(form, std::memory_order_relaxed);
  return LVKV_OK;
}

int lvkv_device_groups(void) {
  int rc = LVKV_OK;
  DeviceCtx* c = current_ctx(&rc);
  return c ? c->groups : rc;
}

}  // extern "C"
