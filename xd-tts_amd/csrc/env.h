// env.h -- every environment variable libxdtts_hip.so reads.  env.cpp holds the table (name, class, moment of reading) and
// is the only file of the library that reads the environment; DESIGN_NOTES.md Appendix B lists the same names (a test compares the two).
#pragma once
#include <cstdlib>

namespace xdtts {
namespace env {

enum Id {
  DEVICE, CHIP_LOCK_DIR, DECODER, GL, COOP,                                  // product
  ATT_FUSED, NO_EARLY, NO_TAIL, NO_CTXFOLD, NO_SKEW, P8,                     // engine forms (the tests compare them)
  GEMM_TILE, GEMM_SPLITK, GEMM_SPLIT_TILE, GL_BATCH_FORCE, PROSODY_BATCH, LOUD,
  ATT_SPINS, ATT_FAULT, ATT_SLOW, TAIL_FAULT,                                // test hooks of the lost / slow workgroup paths
  PERSIST_SPINS, PERSIST_FAULT, PERSIST_SLOW, ENC_SPINS, ENC_FAULT, GL_SPINS, GL_SLOW,
  PERSIST_PROFILE, GL_PROFILE,                                               // output paths of the `make prof` build
  N_VARS
};
enum class Kind { product, form, hook };
enum class When { process, handle, request };  // read once per process / when a handle is created / in every request
struct Var {
  const char *name;
  Kind kind;
  When when;
};
extern const Var table[N_VARS];

const char *raw(Id id);              // the value, or null
bool is_set(Id id);
bool equals(Id id, const char *v);   // set, and exactly v
int int_or(Id id, int unset);
template <class T>
void override_int(Id id, T *v) {     // *v only changes when the variable is set
  if (const char *e = raw(id)) *v = (T)atoi(e);
}
int coop_forced();                   // XDTTS_COOP, once per process: -1 unset, 0 plain launches, 1 cooperative launches

}  // namespace env
}  // namespace xdtts
