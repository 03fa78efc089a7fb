// ORACLE (test infrastructure only) — the leaf functions are the product's headers (rtxpt_amd/csrc/pt_*.h, namespace ptk): one text, included by both.
// Everything under oracle/ includes this file first, so that ptref:: finds ptk's names.
#pragma once
#include "../../rtxpt_amd/csrc/pt_vec.h"
namespace ptref { using namespace ptk; }
