// Hold<T>: a variable takes a value for one scope.  The constructor stores what the variable held and assigns the new value; the destructor
// puts the stored value back -- on every way out of the scope, the early `return` of MX(...) / HIPX(...) included.  Plain C++, no HIP.
#pragma once

namespace mimrl {

template <typename T> struct hold_value { using type = T; };   // keeps the value out of template deduction: Hold h(flag, 1) holds flag's own type

template <typename T>
class Hold {
 public:
  Hold(T& var, typename hold_value<T>::type value) : var_(var), saved_(var) { var_ = value; }
  ~Hold() { var_ = saved_; }
  Hold(const Hold&) = delete;
  Hold& operator=(const Hold&) = delete;

 private:
  T& var_;
  T saved_;
};

}  // namespace mimrl
