// vaqhip_rccl.h -- RCCL resolved at run time: the function table and its loader (vaqhip_rccl.cpp), and
// nothing of the index.  libvaqhip.so does not link RCCL: the types and the signatures come from
// <rccl/rccl.h>, the addresses from dlopen at the first multi-device search that exchanges over RCCL.
#ifndef VAQHIP_RCCL_H
#define VAQHIP_RCCL_H
#include <rccl/rccl.h>

#include <string>

// (hidden: none of this joins the library's exported symbols)
namespace vaqhost __attribute__((visibility("hidden"))) {

struct Rccl {
  void *h = nullptr;
  decltype(&ncclCommInitAll) CommInitAll = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclAllGather) AllGather = nullptr;
  decltype(&ncclGroupStart) GroupStart = nullptr;
  decltype(&ncclGroupEnd) GroupEnd = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
  std::string where;
};
extern Rccl g_rccl;  // empty until load_rccl has succeeded once

bool load_rccl(std::string *err);

} // namespace vaqhost
#endif
