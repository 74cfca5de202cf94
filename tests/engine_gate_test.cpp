// engine_gate_test.cpp -- the fallback policy of xd-tts_amd/csrc/engine_gate.h on the host alone (no HIP, no GPU): what a GPU
// test cannot reach without 64 demoted requests.  Built and run by tests/test_engine_gate_cpu.py; prints "ok" and exits 0.
#include <cstdio>
#include <cstdlib>

#include "engine_gate.h"

using xdtts::EngineGate;

#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

int main() {
  static_assert(EngineGate::PROBE_AFTER == 64, "the stderr messages and the documents say 64");
  {  // unprobed -> probe passes -> on; the probe runs once
    EngineGate g;
    int probes = 0;
    CHECK(g.abi_state() == -1 && !g.usable());
    CHECK(!g.tick() && g.abi_state() == -1);  // nothing to count before the probe
    g.ensure_probed([&] { ++probes; return true; });
    CHECK(g.usable() && g.abi_state() == 1);
    g.ensure_probed([&] { ++probes; return false; });
    CHECK(probes == 1 && g.usable());
    CHECK(!g.tick() && g.usable() && g.demoted_calls == 0);  // an engine that is on does not count
  }
  {  // demote -> off for 63 ticks, on at the 64th, counter re-armed
    EngineGate g;
    g.ensure_probed([] { return true; });
    for (int round = 0; round < 2; ++round) {
      g.demote();
      CHECK(!g.usable() && g.abi_state() == 0 && g.demoted_calls == 0);
      for (int i = 1; i <= 63; ++i) {
        CHECK(!g.tick());
        CHECK(!g.usable() && g.abi_state() == 0 && g.demoted_calls == i);
      }
      CHECK(g.tick());
      CHECK(g.usable() && g.abi_state() == 1 && g.demoted_calls == 0);
    }
    // a second demotion on the way re-arms the count
    g.demote();
    for (int i = 0; i < 40; ++i) CHECK(!g.tick());
    g.demote();
    for (int i = 0; i < 63; ++i) CHECK(!g.tick());
    CHECK(!g.usable());
    CHECK(g.tick() && g.usable());
  }
  {  // refuse -> off through any number of ticks and through reset()
    EngineGate g;
    g.ensure_probed([] { return true; });
    g.refuse();
    CHECK(!g.usable() && g.abi_state() == 0 && g.refused);
    for (int i = 0; i < 1000; ++i) CHECK(!g.tick());
    CHECK(!g.usable() && g.abi_state() == 0);
    g.reset();
    CHECK(!g.usable() && g.abi_state() == 0 && g.refused);
    int probes = 0;
    g.ensure_probed([&] { ++probes; return true; });  // never probed again
    CHECK(probes == 0 && !g.usable());
    for (int i = 0; i < 1000; ++i) CHECK(!g.tick());
    CHECK(g.abi_state() == 0);
  }
  {  // reset() on a demoted gate -> unprobed, counter cleared; the next probe decides
    EngineGate g;
    g.ensure_probed([] { return true; });
    g.demote();
    for (int i = 0; i < 10; ++i) g.tick();
    g.reset();
    CHECK(g.abi_state() == -1 && !g.usable() && g.demoted_calls == 0);
    g.ensure_probed([] { return true; });
    CHECK(g.usable() && g.abi_state() == 1);
    g.reset();  // ... and on a gate that is on
    CHECK(g.abi_state() == -1);
  }
  {  // a gate whose probe failed never ticks back; reset() lets it be probed again
    EngineGate g;
    g.ensure_probed([] { return false; });
    CHECK(!g.usable() && g.abi_state() == 0);
    for (int i = 0; i < 1000; ++i) CHECK(!g.tick());
    CHECK(!g.usable() && g.abi_state() == 0);
    g.demote();  // (a coupled demotion of an engine the device cannot host)
    for (int i = 0; i < 1000; ++i) CHECK(!g.tick());
    CHECK(g.abi_state() == 0);
    g.reset();
    CHECK(g.abi_state() == -1);
    g.ensure_probed([] { return false; });
    CHECK(g.abi_state() == 0);
  }
  std::puts("ok");
  return 0;
}
