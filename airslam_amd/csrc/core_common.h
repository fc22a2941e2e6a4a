// airfe — what every *_core.h shares: the host/device switch, the count clamp and the three facts about a double that the host statements and the kernels
// must decide alike.  Plain C++17 for the host builds of the cores (tests, tools/*_host_check.cpp); under hipcc the same text is host and device code.
#ifndef AIRFE_CORE_COMMON_H_
#define AIRFE_CORE_COMMON_H_

#if defined(__HIPCC__) || defined(__HIP__)
#define AIRFE_HD __host__ __device__ inline
#else
#define AIRFE_HD inline
#endif

// a stored count as every reader clamps it: into [0, cap]
AIRFE_HD int clamp_count(int n, int cap) { return n < 0 ? 0 : (n > cap ? cap : n); }

// Written as comparisons of the value with itself, not as library calls: the expressions are the contract (compiled with -ffp-contract=off on both sides).
AIRFE_HD bool is_finite(double v) { return v - v == 0.0; }
AIRFE_HD bool is_nan(double v) { return v != v; }
AIRFE_HD double quiet_nan() { return __builtin_nan(""); }
// any NaN -> the one quiet NaN whose bits the host statement writes
AIRFE_HD double canon_nan(double v) { return v != v ? __builtin_nan("") : v; }

#endif  // AIRFE_CORE_COMMON_H_
