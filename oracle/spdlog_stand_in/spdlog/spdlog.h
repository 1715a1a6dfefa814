// oracle/spdlog_stand_in/spdlog/spdlog.h -- TEST INFRASTRUCTURE ONLY.
// Stand-in for spdlog (see common.h in this directory for why it exists; it
// must never be on an include path of the product).  A logger that discards
// everything it is given.
#pragma once
#include <memory>
#include <string>

#include "common.h"

namespace spdlog {

class logger {
 public:
  logger() = default;
  explicit logger(std::string name) : name_(std::move(name)) {}
  template <class... A> void trace(A &&...) {}
  template <class... A> void debug(A &&...) {}
  template <class... A> void info(A &&...) {}
  template <class... A> void warn(A &&...) {}
  template <class... A> void error(A &&...) {}
  template <class... A> void critical(A &&...) {}
  template <class... A> void log(A &&...) {}
  void set_level(level::level_enum) {}
  void flush() {}
  const std::string &name() const { return name_; }

 private:
  std::string name_;
};

}  // namespace spdlog
