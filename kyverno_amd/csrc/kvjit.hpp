// Specialized kernels: the compiled policy set (bytecode, predicates, globs) is
// lowered once more, to HIP C++ with every rule as straight-line device code
// (constants as immediates, cursors in registers, per-lane control flow done by
// the hardware exec mask instead of the interpreter's uniform-pc emulation),
// and compiled for gfx950 with hiprtc when the policy set is compiled.
#pragma once
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "kvinternal.hpp"
#include "kvdevtypes.h"

namespace kvh {

struct JitChunk {
  std::vector<uint32_t> rules;  // the rules evaluated by kernel `name`
  std::string name;
};

// One specialized rule kernel: rules [first, first + count) of the signature-sorted
// rule order as consecutive fused blocks of `blocks[i]` rules (sum = count), compiled with
// a `waves`-per-SIMD launch bound (0: none). Every array a block's rules walk is walked
// once per resource and block; the rules of a block keep their state in registers across
// the whole block, so the block sizes bound the kernel's register use.
struct JitKernelPlan {
  uint32_t first, count;
  int waves;
  std::vector<uint32_t> blocks;
  // its hoist regions in three parts (cell loads, word gathers, array fix-up) instead of first-use
  // order: more loads in flight, more registers live. The first plan asks for it; the build keeps
  // it for the kernels that meet their register rules with it at the plan they settle on in
  // first-use order (kvjitbuild.cpp jit_group_regions)
  bool grouped = false;
  // its per-rule and nested array loops over path columns (kvjitgen.cpp ColLoop) instead of walking
  // the node rows: a hoist region more per loop. Asked for and kept as `grouped` is, and given up
  // before it (jit_group_regions)
  bool colloops = false;
};

struct JitImage {
  std::vector<JitKernelPlan> plan;     // kernel grouping (empty: default groups; kept across re-plans)
  std::string source;       // generated HIP source, all of it (diagnostics, tools/kvemu)
  std::string common;       // prelude + helper functions shared by the kernels
  std::vector<std::string> kernel_name, kernel_src;  // one hiprtc program per kernel: common + kernel_src[i]
  std::vector<std::vector<char>> codes;              // gfx950 code object per kernel program
  std::vector<JitChunk> chunks;
  // leaf predicates memoized per distinct scalar value: slot k = memo_preds[k];
  // kernel "kvj_ptab" fills DevPS::ptab (memo_words words per value)
  std::vector<uint32_t> memo_preds;
  uint32_t memo_words = 0;
  uint32_t ptab_row = 1;    // predicates per kvj_ptab grid row (one row: every predicate of a value)
  // match bits per tuple (kv_mtup_kernel, DevPS::mtup): words of 32 rules in kernel order,
  // from the factored-match descriptors (DevPS::fac_*, kvjitgen.cpp build_fac)
  uint32_t mtup_words = 0;
  std::vector<uint32_t> fac_word, fac_bit, fac_flist, fac_rule;
  uint32_t fac_slots = 0;
  // per rule: 1 = its records are appended to its wave's 64-slot segment (lane in the record),
  // 0 = at the resource's slot (members of large rule groups, kvjitgen.cpp kGslotMembers; members of
  // groups with site records, expanded there at fetch)
  std::vector<uint8_t> rec_compact;
  // site-record groups (kvdevtypes.h GSiteDesc): 4 words per group, (rule, node shift) per member,
  // members in all
  std::vector<uint32_t> gs_desc, gs_mem;
  uint32_t gs_members = 0;
  // path columns the kernels read (kvdevtypes.h ColDesc, built per batch by kvcol.h): every
  // column; per family its array's column (an index into cols: of family 0, or of the parent
  // family of a nested one), its parent family (0: none) and its column count
  std::vector<kv::ColDesc> cols;
  std::vector<uint32_t> fam_arr, fam_parent, fam_ncols;
  // per family its wide columns, those of them with a b plane, and its narrow columns (cell
  // formats: kvdevtypes.h ColFmt; KVGPU_JIT_NARROW=0 at generation: every column wide)
  std::vector<uint32_t> fam_nw, fam_nb, fam_nn;
  // what the kernels read of each column ("<family array path>|<relative path>" -> use bits,
  // kvjitgen.cpp Gen::ColUse): the formats follow from the uses of every rule of the policy set, so
  // an image that generates only some rules (a block probe) is seeded with the whole image's
  std::map<std::string, uint32_t> col_use;
  bool probe = false;      // a block-probe image (jit_refine_blocks): rule kernels only
  double gen_ms = 0, compile_ms = 0;
  // Output-mode variants (jit_compile_variants): the final plan's rule kernels compiled once more
  // per DevOut::full value the benchmarks and callers run most (KVJ_FULL a constant), so a kernel
  // carries no code for outputs its launches never write. codes[i] is program i's variant; empty
  // where the program is not a rule kernel or its variant spilled (the generic code runs there).
  struct Variant {
    uint32_t full = 0;
    std::vector<std::vector<char>> codes;
  };
  std::vector<Variant> variants;
};

// ---- kvjitgen.cpp
// most rules per kernel (one fused block): KVGPU_JIT_CHUNK, default 128
uint32_t jit_chunk_rules();
// diagnostics (KVGPU_JIT_STAMPS): stamps per wave of the rule kernels' segment boundaries
constexpr uint32_t kJitStamps = 16;
// Generate the specialized source for every rule of `ps` (kernels of at most `chunk_rules` rules).
void jit_generate(const PolicySet& ps, uint32_t chunk_rules, JitImage* out);

// ---- kvjitbuild.cpp
// The whole build of a policy set's kernels into a fresh `img`: generate, the plan (from the plan
// cache, or block sizes from probe compiles), compile / re-plan rounds until every kernel meets the
// register rules, the output-mode variants, the plan cache entry; img->compile_ms: every compile on
// the way. KVGPU_JIT_DUMP / _DUMP_CO: the source / the code objects to files; _SKIP_COMPILE: no compile.
void jit_build(const PolicySet& ps, JitImage* img);
uint64_t code_bytes(const JitImage& img);
// Does a compiled kernel meet the register rules? One verdict for the spill plan, the variants
// and the block probes, from the kernel descriptor's private segment and VGPR count, the bound of
// `waves` per SIMD it was compiled under (0: none) and whether it calls kv_dleaf_impl (the
// out-of-line dynamic-leaf evaluator of pattern variables, which keeps a call frame in scratch).
struct RegVerdict {
  uint32_t priv, vgprs;
  bool calls;
  bool fits;        // within the bound's registers: vgprs <= 512 / waves
  bool scratch_ok;  // no private segment, or the call frame in a kernel without a bound (the round-1
                    // fault was spill code under a bound)
  bool ships() const { return fits && scratch_ok; }  // a planned kernel is kept, a variant ships
  // A block probe splits its block. Deliberately not !ships(): a probe always has a bound, and the
  // call frame is excused there too (the spill plan drops such a kernel's bound, blocks untouched).
  bool probe_splits() const { return (priv != 0 && !calls) || !fits; }
};
RegVerdict reg_verdict_of(uint32_t priv, uint32_t vgprs, int waves, bool calls);
// Register budget of the plan, from the verdict of each planned kernel: a kernel that ships is kept;
// one whose only fault is a call frame under a bound drops the bound. Otherwise a multi-block kernel
// under a bound of w > 6 waves per SIMD is recompiled at w - 1; else its largest block is split in
// two; a kernel of one-rule blocks is compiled at w - 1, then without a bound, then as two kernels
// (a one-rule kernel that still spills: std::runtime_error). Returns true when the plan changed
// (regenerate + compile again; the kernels that did not change come from the code-object cache).
bool jit_plan_spills(JitImage* img, const std::vector<RegVerdict>& verdicts);
// Plan cache (in the code-object cache directory): the final kernel plan of a policy set,
// keyed by a hash of its first generated image, so a later compile of the same set goes
// straight to its final kernels (plan-<key>.txt, which also lists their code-object files).
bool jit_load_plan(const std::string& key, JitImage* img);
void jit_save_plan(const std::string& key, const JitImage& img);

}  // namespace kvh
