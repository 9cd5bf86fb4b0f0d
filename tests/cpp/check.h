// The failure count and CHECK of the stand-alone check programs in this directory: a failed check is
// reported with its place and counted, and the program goes on; main returns 1 if g_failed is set.
#pragma once

#include <cstdio>

inline int g_failed = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                            \
    }                                                                        \
  } while (0)
