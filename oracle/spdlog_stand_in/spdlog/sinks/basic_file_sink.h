// oracle/spdlog_stand_in/spdlog/sinks/basic_file_sink.h -- TEST INFRASTRUCTURE ONLY.
// Stand-in for spdlog (see ../common.h; never on an include path of the
// product).  No sink is needed: the stand-in logger discards everything.
#pragma once
#include "../spdlog.h"
