// a-loam_amd/csrc/capi_range.hip — host side of range-image input: the decoder (aloam_set_range_decoder) and the four entries that hand sweeps over
// as 16-bit range images.  They differ from their float-record twins (capi_odometry.hip) only in what they check and in which two kernels read the
// sweep; the staging slabs, the copy stream and everything behind the front end are shared (register_launch, stage_batch).
#include <algorithm>
#include <cstring>
#include <vector>

#include "capi_internal.hpp"

namespace {

size_t blob_bytes(const aloam_ctx* c, int n_cols) { return 2 * ((((size_t)n_cols + 7) & ~(size_t)7) + (size_t)n_cols * c->rd_rows); }

// A batch of range images, checked before anything of it is queued; points[b] = n_cols[b] * rows.
int check_range_batch(aloam_ctx* c, const void* sweeps, const int* n_cols, std::vector<int>* points) {
  if (!c) return ALOAM_E_ARG;
  if (!sweeps || !n_cols) { c->err = "null sweeps / n_cols"; return ALOAM_E_ARG; }
  if (const int rc = require_stage(c, ALOAM_STAGE_REGISTRATION)) return rc;
  if (!c->range_on) { c->err = "range-image input before aloam_set_range_decoder"; return ALOAM_E_STATE; }
  points->resize(c->B);
  for (int b = 0; b < c->B; ++b) {
    if (n_cols[b] < 0) { c->err = "negative column count (n_cols)"; return ALOAM_E_ARG; }
    if ((long long)n_cols[b] * c->rd_rows > c->max_points) { c->err = "n_cols * rows exceeds max_points"; return ALOAM_E_CAPACITY; }
    (*points)[b] = n_cols[b] * c->rd_rows;
  }
  return ALOAM_OK;
}

int register_range_device(aloam_ctx* c, const void* d_sweeps, long long seq_stride_bytes, const int* n_cols, bool debug_arrays) {
  std::vector<int> points;
  if (const int rc = check_range_batch(c, d_sweeps, n_cols, &points)) return rc;
  if (((size_t)d_sweeps & 1) || (seq_stride_bytes & 1)) { c->err = "range images must be 2-byte aligned (d_sweeps, seq_stride_bytes)"; return ALOAM_E_ARG; }
  return register_launch(c, d_sweeps, seq_stride_bytes, points.data(), 2, -1, debug_arrays, n_cols);
}

int register_range_host(aloam_ctx* c, const void* h_sweeps, long long seq_stride_bytes, const int* n_cols, bool debug_arrays) {
  std::vector<int> points;
  int rc = check_range_batch(c, h_sweeps, n_cols, &points);
  if (rc) return rc;
  // a slab row holds the largest blob max_points allows (the header is longest with one row per column), rounded to 16 bytes
  const size_t d_seq_stride = (2 * ((((size_t)c->max_points + 7) & ~(size_t)7) + (size_t)c->max_points) + 15) & ~(size_t)15;
  int slot = 0;
  char* d_in = nullptr;
  if ((rc = stage_batch(c, h_sweeps, seq_stride_bytes, blob_bytes(c, *std::max_element(n_cols, n_cols + c->B)), blob_bytes(c, n_cols[c->B - 1]), d_seq_stride, &slot, &d_in))) return rc;
  return register_launch(c, d_in, (long long)d_seq_stride, points.data(), 2, slot, debug_arrays, n_cols);
}

}  // namespace

extern "C" {

int aloam_set_range_decoder(aloam_ctx* c, const aloam_range_decoder* d) {
  DeviceScope device_scope(c);
  if (!c) return ALOAM_E_ARG;
  if (!d) { c->err = "null decoder"; return ALOAM_E_ARG; }
  if (const int rc = require_stage(c, ALOAM_STAGE_REGISTRATION)) return rc;
  if (d->rows < 1 || d->rows > kMaxRings) { c->err = "decoder: rows must be in 1 .. 128"; return ALOAM_E_ARG; }
  if (d->n_az < 1 || d->n_az > 65536) { c->err = "decoder: n_az must be in 1 .. 65536"; return ALOAM_E_ARG; }
  if (d->order != ALOAM_RANGE_COLUMN_MAJOR && d->order != ALOAM_RANGE_ROW_MAJOR) { c->err = "decoder: order must be ALOAM_RANGE_COLUMN_MAJOR or ALOAM_RANGE_ROW_MAJOR"; return ALOAM_E_ARG; }
  if (!d->az_x || !d->az_y || !d->cos_el || !d->sin_el || !d->range_off || !d->z_off || !d->az_off || !d->ring_id) { c->err = "decoder: null table (az_x, az_y, cos_el, sin_el, range_off, z_off, az_off, ring_id)"; return ALOAM_E_ARG; }
  for (int r = 0; r < d->rows; ++r) {
    if (d->az_off[r] <= -d->n_az || d->az_off[r] >= d->n_az) { c->err = "decoder: |az_off| must be below n_az (row " + std::to_string(r) + ")"; return ALOAM_E_ARG; }
    if (d->ring_id[r] < -1 || d->ring_id[r] >= c->R) { c->err = "decoder: ring_id must be -1 or in 0 .. n_scans-1 (row " + std::to_string(r) + ")"; return ALOAM_E_ARG; }
  }
  std::vector<float2> az(d->n_az);
  for (int a = 0; a < d->n_az; ++a) az[a] = make_float2(d->az_x[a], d->az_y[a]);
  std::vector<float> tab((size_t)kRangeRowTables * kMaxRings, 0.f);            // [table][row], the order of kRangeRowTables
  for (int r = 0; r < d->rows; ++r) {
    tab[0 * kMaxRings + r] = d->cos_el[r]; tab[1 * kMaxRings + r] = d->sin_el[r]; tab[2 * kMaxRings + r] = d->range_off[r]; tab[3 * kMaxRings + r] = d->z_off[r];
    std::memcpy(&tab[4 * kMaxRings + r], &d->az_off[r], sizeof(int));
    tab[5 * kMaxRings + r] = (float)d->ring_id[r];
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));                                 // a registration in flight still reads the tables in force
  c->range_on = false;
  c->d_rd_az.reset();
  HIP_TRY(c, dalloc(c->d_rd_az, az.size()));
  if (!c->d_rd_rows) HIP_TRY(c, dalloc(c->d_rd_rows, tab.size()));
  HIP_TRY(c, hipMemcpy(c->d_rd_az.get(), az.data(), sizeof(float2) * az.size(), hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(c->d_rd_rows.get(), tab.data(), sizeof(float) * tab.size(), hipMemcpyHostToDevice));
  c->rd_rows = d->rows; c->rd_n_az = d->n_az; c->rd_order = d->order; c->rd_scale = d->range_scale;
  c->range_on = true;
  return ALOAM_OK;
}

int aloam_scan_register_range_device(aloam_ctx* c, const void* d_sweeps, long long seq_stride_bytes, const int* n_cols) {
  DeviceScope device_scope(c);
  return register_range_device(c, d_sweeps, seq_stride_bytes, n_cols, true);
}

int aloam_scan_register_range_host(aloam_ctx* c, const void* h_sweeps, long long seq_stride_bytes, const int* n_cols) {
  DeviceScope device_scope(c);
  return register_range_host(c, h_sweeps, seq_stride_bytes, n_cols, true);
}

int aloam_process_range_device(aloam_ctx* c, const void* d_sweeps, long long seq_stride_bytes, const int* n_cols) {
  DeviceScope device_scope(c);
  if (const int rc = register_range_device(c, d_sweeps, seq_stride_bytes, n_cols, false)) return rc;
  return aloam_odometry_step(c);
}

int aloam_process_range_host(aloam_ctx* c, const void* h_sweeps, long long seq_stride_bytes, const int* n_cols) {
  DeviceScope device_scope(c);
  if (const int rc = register_range_host(c, h_sweeps, seq_stride_bytes, n_cols, false)) return rc;
  return aloam_odometry_step(c);
}

}  // extern "C"
