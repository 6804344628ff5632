// error.h -- the thread-local error slot behind bm_last_error_string() and the HIP error check every host file reports through
#pragma once
#include <hip/hip_runtime.h>

#include <string>

namespace bm {

void set_error(const std::string& msg);
const char* last_error();
int hip_fail(hipError_t e, const char* what, const char* file, int line);

#define BM_HIP(expr)                                                        \
	do {                                                                    \
		hipError_t bm_e_ = (expr);                                          \
		if (bm_e_ != hipSuccess) return ::bm::hip_fail(bm_e_, #expr, __FILE__, __LINE__); \
	} while (0)

} // namespace bm
