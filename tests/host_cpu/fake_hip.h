// fake_hip.h -- what the image check's driver may ask the CPU device fake
// (fake_hip.cpp, fake_launch.cpp) besides the hip* and tmx::launch_* symbols
// tm_host.cpp links against.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../emqx_amd/csrc/tm_dev.h"

extern "C" {
// the next k hipEventQuery calls answer hipErrorNotReady (0: none)
void fake_hip_busy_events(uint64_t k);
// bytes of the live "device" or pinned allocation that starts at p (0: not one)
size_t fake_hip_alloc_bytes(const void *p);
// bytes left from p to the end of the live allocation holding it (0: in none)
size_t fake_hip_room(const void *p);
// live allocations (a leak check at exit)
size_t fake_hip_live_allocs(void);
}

namespace fake {
// the last view a match launch was given (valid: a launch has run)
const tmx::DevIndex &last_view();
bool have_view();
// answers of small_path_ok for batches of 1 .. 65536 topics
void set_small_ok(bool on);
// launches served so far, per launcher
struct Counts { uint64_t match, pairs, first, small_segs, patch, patch_runs, mfilter, sort, unsupported; };
Counts counts();
}  // namespace fake
