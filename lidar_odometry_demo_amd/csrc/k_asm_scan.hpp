// How a kernel reads its scan's descriptor, shared by the map assembly (k_assemble.hpp) and the scan votes (k_vote.hpp).
// A launch is a grid (workgroups of the largest scan, scans): blockIdx.y names the scan, whose descriptor is read through
// the constant address space (scalar loads, like kernel arguments).  No kernel here, so that more than one translation
// unit can include it.
#pragma once
#include <hip/hip_runtime.h>

#include "assemble_host.hpp"

namespace lom {

using assemble::AsmScan;
using assemble::kAsmThreads;

typedef const __attribute__((address_space(4))) AsmScan *ConstAsm;  // read with scalar loads, like kernel arguments

}  // namespace lom
