// env.cpp -- the table of environment variables; nothing else in the library reads the environment (env.h).
#include "env.h"

#include <cstring>

namespace xdtts {
namespace env {

const Var table[N_VARS] = {
    // what a deployment may set
    {"XDTTS_DEVICE", Kind::product, When::handle},          // the process's default GPU
    {"XDTTS_CHIP_LOCK_DIR", Kind::product, When::process},  // cross-process flock per GPU
    {"XDTTS_DECODER", Kind::product, When::request},        // =launch: the launch-per-stage decoder
    {"XDTTS_GL", Kind::product, When::request},             // =launch: the launch-per-iteration vocoder
    {"XDTTS_COOP", Kind::product, When::process},           // 0 / 1: plain / cooperative launches of the co-resident grids
    // second forms of the same arithmetic: the fallback targets, and what the agreement tests compare
    {"XDTTS_ATT_FUSED", Kind::form, When::handle},
    {"XDTTS_NO_EARLY", Kind::form, When::handle},
    {"XDTTS_NO_TAIL", Kind::form, When::handle},
    {"XDTTS_NO_CTXFOLD", Kind::form, When::handle},
    {"XDTTS_NO_SKEW", Kind::form, When::handle},
    {"XDTTS_P8", Kind::form, When::handle},
    {"XDTTS_GEMM_TILE", Kind::form, When::process},
    {"XDTTS_GEMM_SPLITK", Kind::form, When::process},
    {"XDTTS_GEMM_SPLIT_TILE", Kind::form, When::process},
    {"XDTTS_GL_BATCH_FORCE", Kind::form, When::request},
    {"XDTTS_PROSODY_BATCH", Kind::form, When::request},     // =loop: the batch parity hook runs one k_prosody launch per utterance
    {"XDTTS_LOUD", Kind::form, When::request},              // =fp32: the loudness stage's recurrences in fp32 (what fp64 costs)
    // test hooks: a lost or a slow workgroup, a short spin budget
    {"XDTTS_ATT_SPINS", Kind::hook, When::request},
    {"XDTTS_ATT_FAULT", Kind::hook, When::request},
    {"XDTTS_ATT_SLOW", Kind::hook, When::request},
    {"XDTTS_TAIL_FAULT", Kind::hook, When::request},
    {"XDTTS_PERSIST_SPINS", Kind::hook, When::request},
    {"XDTTS_PERSIST_FAULT", Kind::hook, When::request},
    {"XDTTS_PERSIST_SLOW", Kind::hook, When::request},
    {"XDTTS_ENC_SPINS", Kind::hook, When::request},
    {"XDTTS_ENC_FAULT", Kind::hook, When::request},
    {"XDTTS_GL_SPINS", Kind::hook, When::request},
    {"XDTTS_GL_SLOW", Kind::hook, When::request},
    // `make prof` build only: where the in-kernel phase clocks are written
    {"XDTTS_PERSIST_PROFILE", Kind::hook, When::request},
    {"XDTTS_GL_PROFILE", Kind::hook, When::request},
};

const char *raw(Id id) { return getenv(table[id].name); }
bool is_set(Id id) { return raw(id) != nullptr; }
bool equals(Id id, const char *v) {
  const char *e = raw(id);
  return e && std::strcmp(e, v) == 0;
}
int int_or(Id id, int unset) {
  const char *e = raw(id);
  return e ? atoi(e) : unset;
}
int coop_forced() {
  static const int forced = [] {
    const char *e = raw(COOP);
    return !e ? -1 : (e[0] == '0' ? 0 : 1);
  }();
  return forced;
}

}  // namespace env
}  // namespace xdtts
