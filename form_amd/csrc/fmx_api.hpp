// fmx_api.hpp — what the two host units of the C ABI share: fmx_api.cpp (the context, the
// stages, register_scan) and dense_api.cpp (the dense voxel map's entry points).  Included by
// those two only.
#pragma once
#include <exception>
#include <new>

#include "fmx_internal.hpp"

namespace fmx {

// ---- fmx_api.cpp
// every stream of the context: main, side (map build), side2 (pipelined extraction), lin
void sync_all(fmx_ctx* c);
// A deferred fmx_match (ctx->lazy): launched now, before anything reads or changes
// the state it depends on.
void settle_match(fmx_ctx* c);

// ---- dense_api.cpp: the four calls register_scan makes (each described where it is defined)
void dense_settle(fmx_ctx* c);
uint32_t dense_queue(fmx_ctx* c, const float4* d, size_t n, const double* pose34, uint64_t scan_idx);
void dense_finish(fmx_ctx* c, uint32_t flag, fmx_dense_counts* out);
void roll_on_register(fmx_ctx* c, uint64_t j, const double p[3], bool due, size_t n);

// SETTLE: run a deferred fmx_match first — every entry point but fmx_match itself,
// fmx_linearize_matched (which may consume it fused) and those that read no match
// state (pose, stats, profile counters, fmx_sync, the dense map: a deferred match is no
// queued work)
template <bool SETTLE = true, class F>
fmx_status guard(fmx_ctx* c, F&& f) {
  if (!c) return FMX_E_INVAL;
  try {
    FMX_HIP(hipSetDevice(c->device));
    if constexpr (SETTLE) settle_match(c);
    f();
    c->err.clear();
    return FMX_OK;
  } catch (const StatusError& e) {
    c->err = e.what();
    return e.st;
  } catch (const HipError& e) {
    c->err = e.what();
    return FMX_E_HIP;
  } catch (const std::bad_alloc&) {
    c->err = "host allocation failed";
    return FMX_E_OOM;
  } catch (const std::exception& e) {
    c->err = e.what();
    return FMX_E_INVAL;
  }
}

}  // namespace fmx
