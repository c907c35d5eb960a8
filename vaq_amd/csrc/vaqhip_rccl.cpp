// vaqhip_rccl.cpp -- the dlopen loader of vaqhip_rccl.h.
//
// RCCL is loaded at the first multi-device search that needs it: inside a Python process PyTorch's own
// copy is already mapped and is the one that gets used.
#include "vaqhip_rccl.h"

#include <dlfcn.h>

#include <mutex>

namespace vaqhost {

Rccl g_rccl;
static std::mutex g_rccl_mu;

bool load_rccl(std::string *err) {
  std::lock_guard<std::mutex> lk(g_rccl_mu);
  if (g_rccl.h) return true;
  const char *names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so.1"};
  void *h = nullptr;
  for (const char *n : names)  // a copy that is already mapped (PyTorch's) wins
    if ((h = dlopen(n, RTLD_NOW | RTLD_NOLOAD))) { g_rccl.where = std::string(n) + " (already loaded)"; break; }
  if (!h)
    for (const char *n : names)
      if ((h = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) { g_rccl.where = n; break; }
  if (!h) {
    *err = std::string("RCCL not found: ") + dlerror();
    return false;
  }
  Rccl r;
  r.h = h;
  r.where = g_rccl.where;
  // (a field has the type of the function it is named after: decltype(&nccl##name) in the header)
#define VAQ_SYM(name)                                                             \
  r.name = reinterpret_cast<decltype(r.name)>(dlsym(h, "nccl" #name));            \
  if (!r.name) { *err = std::string("RCCL symbol missing: ") + "nccl" #name; return false; }
  VAQ_SYM(CommInitAll)
  VAQ_SYM(CommDestroy)
  VAQ_SYM(AllGather)
  VAQ_SYM(GroupStart)
  VAQ_SYM(GroupEnd)
  VAQ_SYM(GetErrorString)
#undef VAQ_SYM
  g_rccl = r;
  return true;
}

} // namespace vaqhost
