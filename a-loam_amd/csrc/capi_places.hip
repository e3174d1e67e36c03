// a-loam_amd/csrc/capi_places.hip — host side of place recognition: the store and its capacity, the descriptors made on first use, the
// stream-ordered add / match / export / load / clear.  Every argument is checked before anything is queued.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "capi_internal.hpp"

static int require_places(aloam_ctx* c) {
  if (const int rc = require_stage(c, ALOAM_STAGE_REGISTRATION)) return rc;
  if (!c->places_on) { c->err = "place recognition is not enabled (aloam_places_enable)"; return ALOAM_E_STATE; }
  return ALOAM_OK;
}

// The listed sequences each hold a registered sweep (a host flag: nothing is queued otherwise).
static int check_listed(aloam_ctx* c, const int* seqs, int n) {
  if (const int rc = check_ids(c, seqs, n)) return rc;
  for (int i = 0; i < n; ++i)
    if (!c->seq[seqs[i]].has_sweep) {
      c->err = "sequence " + std::to_string(seqs[i]) + " has registered no sweep since it was created, reset or loaded: nothing to describe";
      return ALOAM_E_STATE;
    }
  return ALOAM_OK;
}

// The positive cells a load accepts: inside this range the f32 square of a cell and the sum of 20 of them are normal numbers, so a column
// with a non-zero cell has a positive finite norm (place_column_norm) and counts as non-zero, as the header says.  Below it the squares
// underflow and the column would lose its mask bit; above it the norm is inf and the column would count with cosine 0.
static constexpr float kPlaceCellMin = 0x1p-62f, kPlaceCellMax = 0x1p60f;

// k_place_descriptor for the listed sequences whose current sweep has none yet: at most once per registered sweep.
static int ensure_descriptors(aloam_ctx* c, const int* seqs, int n) {
  std::vector<int> wanted(c->B, 0);
  bool any = false;
  for (int i = 0; i < n; ++i) if (!c->seq[seqs[i]].desc_valid) { wanted[seqs[i]] = 1; any = true; }
  if (!any) return ALOAM_OK;
  if (const int rc = stage_ints(c, wanted.data(), c->B, c->d_pl_wanted.get())) return rc;
  PlaceDescArgs a{};
  a.B = c->B; a.R = c->R; a.slab = c->slab; a.slabs = c->d_slabs.get(); a.ringstart = c->d_ringstart.get(); a.wanted = c->d_pl_wanted.get();
  a.ring_scale = (float)kPlaceRings / c->pl_max_range; a.height = c->pl_height; a.desc = c->d_pl_desc.get();
  launch_place_descriptor(a, c->stream);
  HIP_TRY(c, hipGetLastError());
  on_descriptors_made(c, seqs, n);
  return ALOAM_OK;
}

extern "C" {

int aloam_places_enable(aloam_ctx* c, int capacity, float max_range, float sensor_height) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (const int rc = require_stage(c, ALOAM_STAGE_REGISTRATION)) return rc;
  if (c->places_on) { c->err = "place recognition already enabled"; return ALOAM_E_STATE; }
  if (capacity < 1 || capacity > (1 << 20) || !(max_range > 0.f) || !std::isfinite(max_range) || !std::isfinite(sensor_height)) {
    c->err = "bad place store parameters (1 <= capacity <= 2^20, max_range > 0, sensor_height finite)";
    return ALOAM_E_ARG;
  }
  const size_t B = c->B;
  int rc;
  if ((rc = dmalloc(c, c->d_pl_desc, B))) return rc;
  if ((rc = dmalloc(c, c->d_pl_masks, (size_t)capacity))) return rc;
  if (dalloc(c->d_pl_store, (size_t)capacity) != hipSuccess || dalloc(c->d_pl_unit, (size_t)capacity * kPlaceCells) != hipSuccess) {
    (void)hipGetLastError();
    c->err = "place store of " + std::to_string(capacity) + " entries: allocation failed";
    return ALOAM_E_HIP;
  }
  HIP_TRY(c, dalloc(c->d_pl_seqs, B)); HIP_TRY(c, dalloc(c->d_pl_wanted, B)); HIP_TRY(c, dalloc(c->d_pl_lo, B)); HIP_TRY(c, dalloc(c->d_pl_hi, B));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->pl_capacity = capacity; c->pl_count = 0; c->pl_max_range = max_range; c->pl_height = sensor_height;
  on_places_enabled(c);
  c->places_on = true;
  return ALOAM_OK;
}

int aloam_places_add(aloam_ctx* c, const int* seqs, int n) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (const int rc = require_places(c)) return rc;
  if (const int rc = check_listed(c, seqs, n)) return rc;
  if (c->pl_count + n > c->pl_capacity) {
    c->err = "the place store holds " + std::to_string(c->pl_count) + " of " + std::to_string(c->pl_capacity) + " entries: no room for " + std::to_string(n) + " more";
    return ALOAM_E_CAPACITY;
  }
  if (n == 0) return ALOAM_OK;
  if (const int rc = ensure_descriptors(c, seqs, n)) return rc;
  if (const int rc = stage_ints(c, seqs, n, c->d_pl_seqs.get())) return rc;
  PlaceAddArgs a{};
  a.n = n; a.first = c->pl_count; a.seqs = c->d_pl_seqs.get(); a.desc = c->d_pl_desc.get();
  a.odom = c->d_state.get(); a.mapseq = c->map_on ? c->d_mapseq.get() : nullptr;
  a.store = c->d_pl_store.get(); a.unit = c->d_pl_unit.get(); a.masks = c->d_pl_masks.get();
  launch_place_add(a, c->stream);
  HIP_TRY(c, hipGetLastError());
  c->pl_count += n;
  return ALOAM_OK;
}

int aloam_places_match(aloam_ctx* c, const int* seqs, int n, const int* ranges, int T, aloam_place_match* dst) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (const int rc = require_places(c)) return rc;
  if (const int rc = check_listed(c, seqs, n)) return rc;
  if (T < 1 || T > kPlaceMaxT) { c->err = "T must be 1 .. 8"; return ALOAM_E_ARG; }
  if (n > 0 && !ranges) { c->err = "ranges is NULL"; return ALOAM_E_ARG; }
  std::vector<int> lo(std::max(n, 1)), hi(std::max(n, 1));
  int longest = 0;
  for (int i = 0; i < n; ++i) {
    lo[i] = ranges[2 * i]; hi[i] = ranges[2 * i + 1];
    if (lo[i] < 0 || lo[i] > hi[i] || hi[i] > c->pl_count) {
      c->err = "range " + std::to_string(i) + ": need 0 <= lo <= hi <= " + std::to_string(c->pl_count) + " (the entries stored so far)";
      return ALOAM_E_ARG;
    }
    longest = std::max(longest, hi[i] - lo[i]);
  }
  void* d_dst = nullptr;
  if (const int rc = export_target(c, dst, alignof(aloam_place_match), "dst", &d_dst)) return rc;
  if (n == 0) return ALOAM_OK;
  if (const int rc = c->d_pl_pairs.grow(c, std::max(1LL, (long long)n * longest))) return rc;
  if (const int rc = ensure_descriptors(c, seqs, n)) return rc;
  if (const int rc = stage_ints(c, seqs, n, c->d_pl_seqs.get())) return rc;
  if (const int rc = stage_ints(c, lo.data(), n, c->d_pl_lo.get())) return rc;
  if (const int rc = stage_ints(c, hi.data(), n, c->d_pl_hi.get())) return rc;
  PlaceMatchArgs a{};
  a.n = n; a.T = T; a.max_range = longest; a.seqs = c->d_pl_seqs.get(); a.lo = c->d_pl_lo.get(); a.hi = c->d_pl_hi.get();
  a.desc = c->d_pl_desc.get(); a.unit = c->d_pl_unit.get(); a.masks = c->d_pl_masks.get();
  a.pairs = c->d_pl_pairs.get(); a.dst = static_cast<aloam_place_match*>(d_dst);
  launch_place_match(a, c->stream);
  HIP_TRY(c, hipGetLastError());
  return ALOAM_OK;
}

int aloam_places_export(aloam_ctx* c, int first, int count, aloam_place* dst) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (const int rc = require_places(c)) return rc;
  if (first < 0 || count < 0 || first + (long long)count > c->pl_count) { c->err = "entries [first, first + count) must lie inside the store"; return ALOAM_E_ARG; }
  void* d_dst = nullptr;
  if (const int rc = export_target(c, dst, alignof(aloam_place), "dst", &d_dst)) return rc;
  if (count == 0) return ALOAM_OK;
  HIP_TRY(c, hipMemcpyAsync(d_dst, c->d_pl_store.get() + first, sizeof(aloam_place) * (size_t)count, hipMemcpyDefault, c->stream));
  return ALOAM_OK;
}

int aloam_places_load(aloam_ctx* c, const aloam_place* src, int count) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (const int rc = require_places(c)) return rc;
  if (count < 0) { c->err = "negative count"; return ALOAM_E_ARG; }
  if (count == 0) return ALOAM_OK;
  void* d_src = nullptr;
  const CallerMem m = classify_pointer(c, src, &d_src);
  if (!src || m == kMemManaged || m == kMemOtherDevice || (uintptr_t)src % alignof(aloam_place)) {
    c->err = "src must be 8-byte aligned device memory of the context's device, pinned or pageable host memory";
    return ALOAM_E_ARG;
  }
  if (c->pl_count + (long long)count > c->pl_capacity) {
    c->err = "the place store holds " + std::to_string(c->pl_count) + " of " + std::to_string(c->pl_capacity) + " entries: no room for " + std::to_string(count) + " more";
    return ALOAM_E_CAPACITY;
  }
  // every record is validated before anything changes; records in device memory are read back for it
  std::vector<aloam_place> back;
  const aloam_place* h = src;
  if (m == kMemDevice) {
    back.resize((size_t)count);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(back.data(), src, sizeof(aloam_place) * (size_t)count, hipMemcpyDeviceToHost));
    h = back.data();
  }
  for (int i = 0; i < count; ++i) {
    const float* cells = &h[i].cells[0][0];
    for (int k = 0; k < kPlaceCells; ++k)
      if (!std::isfinite(cells[k]) || cells[k] < 0.f || (cells[k] > 0.f && (cells[k] < kPlaceCellMin || cells[k] > kPlaceCellMax))) {
        c->err = "place record " + std::to_string(i) + ": a cell is negative, not finite, or positive outside [2^-62, 2^60]";
        return ALOAM_E_ARG;
      }
  }
  aloam_place* at = c->d_pl_store.get() + c->pl_count;
  // (pageable memory: the runtime stages the copy and has read the source when the call returns)
  HIP_TRY(c, hipMemcpyAsync(at, m == kMemDevice ? d_src : src, sizeof(aloam_place) * (size_t)count, m == kMemDevice ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
  launch_place_finish(c->d_pl_store.get(), c->d_pl_unit.get(), c->d_pl_masks.get(), c->pl_count, count, c->stream);
  HIP_TRY(c, hipGetLastError());
  c->pl_count += count;
  return ALOAM_OK;
}

int aloam_places_clear(aloam_ctx* c) {
  if (!c) return ALOAM_E_ARG;
  if (const int rc = require_places(c)) return rc;
  c->pl_count = 0;                   // later adds overwrite the entries in stream order; nothing on the device depends on the count
  return ALOAM_OK;
}

int aloam_places_info(aloam_ctx* c, int out[4]) {
  if (!c || !out) return ALOAM_E_ARG;
  if (const int rc = require_places(c)) return rc;
  out[0] = c->pl_count; out[1] = c->pl_capacity;
  std::memcpy(&out[2], &c->pl_max_range, 4); std::memcpy(&out[3], &c->pl_height, 4);
  return ALOAM_OK;
}

}  // extern "C"
