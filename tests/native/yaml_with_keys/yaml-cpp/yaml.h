// STAND-IN, NOT yaml-cpp: the node of tests/compile_native/stubs/yaml-cpp/yaml.h with every key PRESENT, for
// tests/native/shim_robust.cpp — a string reads "cauchy", a double 0.125, everything else its zero.
#pragma once
#include <string>
#include <vector>
namespace YAML {
class Node {
 public:
  Node operator[](const std::string&) const { return Node(); }
  bool IsDefined() const { return true; }
  template <typename T>
  T as() const { return T(); }
};
template <>
inline std::string Node::as<std::string>() const { return "cauchy"; }
template <>
inline double Node::as<double>() const { return 0.125; }
}  // namespace YAML
