/*
 * The preprocessor definitions the reference's build system passes on the command line for a Linux / GCC build, as one
 * force-included header (g++ -include): PBRT_NOINLINE holds parentheses and a double underscore that do not survive a
 * shell command line.
 *
 * TEST INFRASTRUCTURE ONLY (oracle/Makefile target `ref_full`).
 */
#ifndef RPF_ORACLE_REF_DEFINES_H
#define RPF_ORACLE_REF_DEFINES_H

#define PBRT_HAVE_ALLOCA_H
#define PBRT_HAVE_MEMORY_H
#define PBRT_HAVE_HEX_FP_CONSTANTS
#define PBRT_HAVE_BINARY_CONSTANTS
#define PBRT_HAVE_CONSTEXPR
#define PBRT_CONSTEXPR constexpr
#define PBRT_HAVE_ALIGNAS
#define PBRT_HAVE_ALIGNOF
#define PBRT_HAVE_ITIMER
#define PBRT_HAVE_NONPOD_IN_UNIONS
#define PBRT_HAVE_MMAP
#define PBRT_NOINLINE __attribute__((noinline))
#define PBRT_HAVE_POSIX_MEMALIGN
#define PBRT_THREAD_LOCAL thread_local

#endif  // RPF_ORACLE_REF_DEFINES_H
