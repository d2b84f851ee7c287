// mfm_env.hpp -- the one place the native code reads its environment switches (DESIGN §9 lists them all).
// A switch is set when the variable exists, whatever its value; numbers are parsed with atoi / atoll / atof.
#pragma once
#include <cstdint>
#include <cstdlib>

namespace mfm {

inline const char *env_str(const char *name) { return std::getenv(name); }  // (nullptr: not set)
inline bool env_flag(const char *name) { return std::getenv(name) != nullptr; }
inline int env_int(const char *name, int dflt) {
  const char *e = std::getenv(name);
  return e ? std::atoi(e) : dflt;
}
inline int64_t env_i64(const char *name, int64_t dflt) {
  const char *e = std::getenv(name);
  return e ? (int64_t)std::atoll(e) : dflt;
}
inline double env_double(const char *name, double dflt) {
  const char *e = std::getenv(name);
  return e ? std::atof(e) : dflt;
}

}  // namespace mfm
