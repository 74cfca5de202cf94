// engine_gate.h -- the one fallback policy behind every engine that needs its grid co-resident (the pair-persistent and the
// persistent MFMA decoder, the cooperative encoder BiLSTM, the one-launch batched attention, the persistent Griffin-Lim):
//   - the engine is probed once (can the device host its grid?) and used while it works;
//   - a timed-out exchange demotes it: the cause (another process holding CUs) may be transient, so it gets another try
//     after PROBE_AFTER eligible calls, or at once after reset();
//   - a cooperative launch the runtime REFUSED is a property of the device: that gate stays off, through ticks and reset().
// Plain host C++, no HIP: tests/engine_gate_test.cpp drives it on a machine without a GPU.
#pragma once

namespace xdtts {

struct EngineGate {
  static constexpr int PROBE_AFTER = 64;
  enum State { UNPROBED = -1, OFF = 0, ON = 1 };
  State state = UNPROBED;
  bool probe_ok = false;  // the device can host the engine: a demotion may be transient
  bool refused = false;   // the runtime refused its launch: never probed again
  int demoted_calls = 0;  // eligible calls since the demotion

  template <class Probe>
  void ensure_probed(Probe &&probe) {
    if (state != UNPROBED) return;
    probe_ok = probe();
    state = probe_ok ? ON : OFF;
  }
  bool usable() const { return state == ON; }
  void demote() {
    state = OFF;
    demoted_calls = 0;
  }
  void refuse() {
    state = OFF;
    probe_ok = false;
    refused = true;
  }
  // one eligible call; true when this call put a demoted engine back on
  bool tick() {
    if (state != OFF || !probe_ok || refused || ++demoted_calls < PROBE_AFTER) return false;
    demoted_calls = 0;
    state = ON;
    return true;
  }
  void reset() {
    if (refused) return;
    state = UNPROBED;
    demoted_calls = 0;
  }
  int abi_state() const { return (int)state; }
};

}  // namespace xdtts
