// oracle/spdlog_stand_in/spdlog/common.h -- TEST INFRASTRUCTURE ONLY.
//
// A stand-in for the third-party spdlog logging library, written for this
// project: no line of it comes from spdlog or from the reference.  The
// reference's src/filter_block.cpp includes monitor_logger.hpp, which includes
// <spdlog/...>; spdlog is not part of the reference and is not vendored here.
// These five headers give the reference's translation units exactly what they
// need to compile -- a level enumeration and a logger whose logging members
// take any arguments and do nothing -- so that oracle/Makefile can compile
// src/filter_block.cpp unmodified into oracle/_ref/libref_filter_block.so.
//
// This directory must NEVER be on an include path of the product
// (adlsm-tree_amd/): only oracle/Makefile's `ref` target names it.
#pragma once

namespace spdlog {
namespace level {
enum level_enum : int { trace = 0, debug, info, warn, err, critical, off, n_levels };
}  // namespace level
}  // namespace spdlog
