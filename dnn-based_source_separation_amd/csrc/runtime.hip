// The library's runtime: the thread-local error and kernel-name slots behind SEP_REQUIRE / SEP_CHECK_LAUNCH / sep_set_kernel (common.hpp), and
// the ABI version.  Every other translation unit needs this one and nothing else of the library.
#include "common.hpp"

static thread_local char g_err[512] = "";
void sep_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* sep_last_error(void) { return g_err; }
static thread_local const char* g_kernel = "";
void sep_set_kernel(const char* name) { g_kernel = name; }
extern "C" const char* sep_last_kernel(void) { return g_kernel; }
extern "C" int sep_version(void) { return SEP_ABI_VERSION; }
