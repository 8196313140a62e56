// hd.h — the two macros of a header that the kernels and a CPU compiler both compile: GS4D_HD marks a function for the host and the device under
// hipcc and is nothing elsewhere; GS4D_UNROLL asks hipcc to unroll the loop that follows.  Include it by a path relative to the including header.
#ifndef GS4D_HD_H
#define GS4D_HD_H
#if defined(__HIPCC__)
#define GS4D_HD __host__ __device__
#define GS4D_UNROLL _Pragma("unroll")
#else
#define GS4D_HD
#define GS4D_UNROLL
#endif
#endif
