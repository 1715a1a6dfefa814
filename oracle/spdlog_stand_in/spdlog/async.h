// oracle/spdlog_stand_in/spdlog/async.h -- TEST INFRASTRUCTURE ONLY.
// Stand-in for spdlog (see common.h in this directory; never on an include
// path of the product).  Nothing of the asynchronous logger is needed.
#pragma once
#include "spdlog.h"
