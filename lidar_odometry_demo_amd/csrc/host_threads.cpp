// The one member of csrc/host_threads.hpp that is not inline.
#include "host_threads.hpp"

namespace lom {

void Pool::start(unsigned part)
{
    workers_.emplace_back([this, part] { run(part); });
}

}  // namespace lom
