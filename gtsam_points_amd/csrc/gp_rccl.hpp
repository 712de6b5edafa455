// gp_rccl.hpp -- RCCL, loaded on demand.  Included by gp_multi.hip alone: the library is opened with dlopen when a multi-batch really spans several devices
// (single-GPU users never load it), and its entry points are declared here, so building the library needs neither RCCL nor its headers.
#pragma once
#include <dlfcn.h>

#include <string>

#include "gp_host.hpp"

// the part of rccl.h this file uses (nccl.h's public ABI: opaque communicator, result / type / op enumerations), so that building the library does not need RCCL's headers
typedef struct ncclComm* ncclComm_t;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclDouble = 8 } ncclDataType_t;  // ncclFloat64
typedef enum { ncclSum = 0 } ncclRedOp_t;

namespace {

struct Rccl {
  void* handle = nullptr;
  ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  bool ok = false;
};

Rccl& rccl() {
  static Rccl r;
  static bool tried = false;
  if (tried) return r;
  tried = true;
  for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
    r.handle = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
    if (r.handle) break;
  }
  if (!r.handle) return r;
  auto sym = [&](const char* n) { return dlsym(r.handle, n); };
  r.CommInitAll = reinterpret_cast<decltype(r.CommInitAll)>(sym("ncclCommInitAll"));
  r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(sym("ncclCommDestroy"));
  r.AllReduce = reinterpret_cast<decltype(r.AllReduce)>(sym("ncclAllReduce"));
  r.AllGather = reinterpret_cast<decltype(r.AllGather)>(sym("ncclAllGather"));
  r.GroupStart = reinterpret_cast<decltype(r.GroupStart)>(sym("ncclGroupStart"));
  r.GroupEnd = reinterpret_cast<decltype(r.GroupEnd)>(sym("ncclGroupEnd"));
  r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(sym("ncclGetErrorString"));
  r.ok = r.CommInitAll && r.CommDestroy && r.AllReduce && r.AllGather && r.GroupStart && r.GroupEnd && r.GetErrorString;
  return r;
}

int nccl_fail(ncclResult_t e, const char* what) { return gp::fail(GP_ERROR_HIP, std::string("RCCL: ") + what + ": " + (rccl().GetErrorString ? rccl().GetErrorString(e) : "?")); }

#define GP_NCCL(expr)                                      \
  do {                                                     \
    ncclResult_t gp_nccl__ = (expr);                       \
    if (gp_nccl__ != ncclSuccess) return nccl_fail(gp_nccl__, #expr); \
  } while (0)

}  // namespace
