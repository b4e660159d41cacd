// Error reporting for the C ABI: functions return an int status; the message of the last failure on
// the calling thread is available through lvc_last_error() (reference behaviour being replaced:
// AT_ASSERTM/AT_ERROR -> C++ exception -> Python RuntimeError, csrc/ROIAlign/ROIAlign_cuda.cu:318-324;
// the Python host re-raises RuntimeError with this text).
#include "conv_common.h"
#include <stdarg.h>
#include <stdlib.h>

static thread_local char g_err[512] = "";

extern "C" void lvc_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}

extern "C" const char* lvc_last_error(void) { return g_err; }

extern "C" int lvc_abi_version(void) { return 1; }

// Range slot of the NEXT fp16-split conv/GEMM launch on this thread: the kernels raise bit 1 of workspace word
// lvc_ws_range_index(slot) (conv_common.h) when an operand leaves their range, so the host can tell WHICH layer it was (slot 0 = the
// shared word).
static thread_local int g_range_slot = 0;
extern "C" void lvc_set_range_slot(int slot) { g_range_slot = (slot > 0 && slot < LVC_RANGE_SLOTS) ? slot : 0; }
extern "C" int lvc_range_slot(void) { return g_range_slot; }
extern "C" int lvc_range_slots(void) { return LVC_RANGE_SLOTS; }

// Compute units of the current device, read once: what the conv / GEMM launchers size their persistent grids by.
extern "C" int lvc_cu_count(void) {
  static int g_cus = 0;
  if (g_cus == 0) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      cus = 256;
    g_cus = cus;
  }
  return g_cus;
}

// Patch decomposition of the 3x3 kernels (patch_plan.h): 0 = one patch shape per map, as before the planner -- the A/B arm and the
// tests' witness; 1 (default) = up to two regions per map in the Winograd kernel, whose outputs do not depend on the patches (bit for
// bit); 2 = in the direct kernel as well, where fewer tiles move the stream-K worker boundaries and with them the last bits of the
// tiles split there -- enough to swap two detections of nearly equal score, so it is not the default.  The environment is looked at
// ONCE, at the first question or setting (LVC_PATCH_PLAN=0/1/2), never on a later launch; the setter overrides it.
static int g_patch_plan = -1;
static void patch_plan_init() {
  if (g_patch_plan >= 0) return;
  const char* e = getenv("LVC_PATCH_PLAN");
  g_patch_plan = (e && (e[0] == '0' || e[0] == '2') && e[1] == 0) ? e[0] - '0' : 1;
}
extern "C" void lvc_set_patch_plan(int mode) { g_patch_plan = mode <= 0 ? 0 : mode >= 2 ? 2 : 1; }
extern "C" int lvc_patch_plan(void) {
  patch_plan_init();
  return g_patch_plan;
}
