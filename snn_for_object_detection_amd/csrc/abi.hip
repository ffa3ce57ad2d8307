// The library's error state and ABI version: the thread-local text behind SNN_REQUIRE / SNN_CHECK_LAUNCH (snn_common.h)
// and the two entry points every caller starts with.  No device code.
#include <stdarg.h>
#include "snn_common.h"

static thread_local char g_err[512] = "";

void snn_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* snn_last_error(void) { return g_err; }
extern "C" int snn_abi_version(void) { return SNN_ABI_VERSION; }
