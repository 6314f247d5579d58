// planner_link.h — what planner.hip needs of a qs_handle beyond the C-ABI (the
// record itself stays private to quadswarm.hip).  Host only.
#pragma once

#include <cstdint>
#include <string>

#include "quadswarm.h"

namespace qs {

struct HandleInfo {
  int device;
  int64_t env_offset;   // global id of env 0
  bool reset_done;      // qs_reset has run
};
void handle_info(const qs_handle* h, HandleInfo* out);

// Sets qs_last_error's thread-local message and returns `code`.
int set_last_error(int code, const std::string& msg);

}  // namespace qs
