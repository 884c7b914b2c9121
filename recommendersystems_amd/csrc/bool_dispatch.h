// f(std::true_type or std::false_type, ...) for runtime bools: one instantiation of f per combination (the kernel launchers
// of iterate.hip and seed_chain.hip)
#pragma once
#include <type_traits>

namespace rwr {

template <class F> static void bool_dispatch(F &&f) { f(); }
template <class F, class... B> static void bool_dispatch(F &&f, bool b, B... bs)
{
    bool_dispatch([&](auto... c) { if (b) f(std::true_type{}, c...); else f(std::false_type{}, c...); }, bs...);
}

}  // namespace rwr
