// jitbuild_check: the build half of the specialized kernels (kyverno_amd/csrc/kvjitbuild.cpp)
// under ASan/UBSan, without a device and without compiling anything. Test infrastructure only
// (tests/test_jitbuild_cpu.py).
//
//   jitbuild_check <empty directory>
//
// checks the register verdict over its domain against the three callers' rules written out, the
// spill plan's ladder on hand-built images with injected verdicts, the plan file's round trip
// in the given directory (as KVGPU_JIT_CACHE), and, on the generator's side (kvjitgen.cpp), that
// every kernel program of a small policy set ends with its own kernel and defines each helper it
// uses before the use. Prints the number of checks; a failed check
// prints its line to stderr and the program exits 1.
#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <stdexcept>

#include "../../kyverno_amd/csrc/kvjit.hpp"

using namespace kvh;

namespace {

int checks = 0, failed = 0;
#define CHECK(c)                                                 \
  do {                                                           \
    checks++;                                                    \
    if (!(c)) {                                                  \
      failed++;                                                  \
      fprintf(stderr, "line %d: %s\n", __LINE__, #c);            \
    }                                                            \
  } while (0)

bool same(const JitKernelPlan& a, const JitKernelPlan& b) {
  return a.first == b.first && a.count == b.count && a.waves == b.waves && a.blocks == b.blocks;
}
bool same(const std::vector<JitKernelPlan>& a, const std::vector<JitKernelPlan>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); i++)
    if (!same(a[i], b[i])) return false;
  return true;
}

// an image of the given kernels (no programs, no code objects: the verdicts are injected)
JitImage image(const std::vector<JitKernelPlan>& plan) {
  JitImage img;
  img.plan = plan;
  for (size_t k = 0; k < plan.size(); k++) img.chunks.push_back({{}, "kvj_r" + std::to_string(plan[k].first)});
  return img;
}

// the plan after one re-plan step of a single kernel with verdict (priv, vgprs, calls)
std::vector<JitKernelPlan> replan(const JitKernelPlan& kp, uint32_t priv, uint32_t vgprs, bool calls, bool* changed) {
  JitImage img = image({kp});
  *changed = jit_plan_spills(&img, {reg_verdict_of(priv, vgprs, kp.waves, calls)});
  return img.plan;
}

void verdict_domain() {
  for (uint32_t priv : {0u, 16u})
    for (int c = 0; c < 2; c++)
      for (int waves : {0, 1, 6, 8})
        for (uint32_t vgprs : {64u, 72u, 88u, 512u}) {
          const bool calls = c != 0;
          const RegVerdict v = reg_verdict_of(priv, vgprs, waves, calls);
          CHECK(v.priv == priv && v.vgprs == vgprs && v.calls == calls);
          // spill plan: keeps the kernel; else drops the bound; else the ladder
          const bool met = waves == 0 || vgprs <= 512u / (uint32_t)waves;
          const bool keep = (priv == 0 || (calls && waves == 0)) && met;
          CHECK(v.ships() == keep);
          const JitKernelPlan kp{0, 8, waves, {5, 3}};
          bool changed = false;
          const std::vector<JitKernelPlan> got = replan(kp, priv, vgprs, calls, &changed);
          const bool dropped = got.size() == 1 && same(got[0], {0, 8, 0, {5, 3}});
          CHECK(changed == !keep);
          if (keep) CHECK(got.size() == 1 && same(got[0], kp));
          else if (calls && met && priv != 0) CHECK(dropped);
          else CHECK(!dropped && !(got.size() == 1 && same(got[0], kp)));
          // variants: ships
          const bool ship = !(priv != 0 && !(calls && waves == 0)) && !(waves > 0 && vgprs > 512u / (uint32_t)waves);
          CHECK(v.ships() == ship);
          // block probes (always under a bound): splits
          if (waves > 0) CHECK(v.probe_splits() == ((priv != 0 && !calls) || vgprs > 512u / (uint32_t)waves));
        }
}

void ladder() {
  bool ch = false;
  std::vector<JitKernelPlan> p;
  // 8 waves, multi-block: gives up a wave
  p = replan({0, 8, 8, {4, 4}}, 16, 64, false, &ch);
  CHECK(ch && p.size() == 1 && same(p[0], {0, 8, 7, {4, 4}}));
  p = replan({0, 8, 8, {4, 4}}, 0, 72, false, &ch);  // (no scratch, over 512 / 8 registers)
  CHECK(ch && p.size() == 1 && same(p[0], {0, 8, 7, {4, 4}}));
  // 6 waves, blocks {5, 3}: the largest block in two halves
  p = replan({0, 8, 6, {5, 3}}, 16, 80, false, &ch);
  CHECK(ch && p.size() == 1 && same(p[0], {0, 8, 6, {2, 3, 3}}));
  // 1 wave, one-rule blocks: without a bound
  p = replan({4, 3, 1, {1, 1, 1}}, 16, 512, false, &ch);
  CHECK(ch && p.size() == 1 && same(p[0], {4, 3, 0, {1, 1, 1}}));
  // (2+ waves, one-rule blocks: one wave fewer)
  p = replan({4, 3, 5, {1, 1, 1}}, 16, 96, false, &ch);
  CHECK(ch && p.size() == 1 && same(p[0], {4, 3, 4, {1, 1, 1}}));
  // 0 waves, 4 one-rule blocks: two kernels of 2 with unit blocks
  p = replan({10, 4, 0, {1, 1, 1, 1}}, 16, 512, false, &ch);
  CHECK(ch && p.size() == 2 && same(p[0], {10, 2, 0, {1, 1}}) && same(p[1], {12, 2, 0, {1, 1}}));
  p = replan({10, 5, 0, {1, 1, 1, 1, 1}}, 16, 512, false, &ch);  // (odd count: 2 + 3)
  CHECK(ch && p.size() == 2 && same(p[0], {10, 2, 0, {1, 1}}) && same(p[1], {12, 3, 0, {1, 1, 1}}));
  // 0 waves, one rule, spilling: an error
  bool threw = false;
  try {
    replan({7, 1, 0, {1}}, 16, 512, false, &ch);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  CHECK(threw);
  // calls, within the bound's registers, scratch, bounded: the bound is dropped, the blocks stay
  p = replan({0, 8, 6, {5, 3}}, 16, 80, true, &ch);
  CHECK(ch && p.size() == 1 && same(p[0], {0, 8, 0, {5, 3}}));
  p = replan({0, 8, 0, {5, 3}}, 16, 80, true, &ch);  // (and is kept so)
  CHECK(!ch && p.size() == 1 && same(p[0], {0, 8, 0, {5, 3}}));
  // several kernels: only those that do not ship change, in place
  JitImage img = image({{0, 8, 6, {5, 3}}, {8, 4, 6, {4}}, {12, 2, 0, {1, 1}}});
  ch = jit_plan_spills(&img, {reg_verdict_of(0, 80, 6, false), reg_verdict_of(0, 88, 6, false), reg_verdict_of(16, 512, 0, false)});
  CHECK(ch && same(img.plan, {{0, 8, 6, {5, 3}}, {8, 4, 6, {2, 2}}, {12, 1, 0, {1}}, {13, 1, 0, {1}}}));
}

void put(const std::string& path, const std::string& text) {
  std::ofstream f(path, std::ios::binary);
  f << text;
}

void plan_file(const std::string& dir) {
  setenv("KVGPU_JIT_CACHE", dir.c_str(), 1);
  JitImage img = image({{0, 8, 6, {2, 3, 3}}, {8, 4, 0, {1, 1, 1, 1}}, {12, 70, 8, {70}}});
  img.common = "// common\n";
  img.kernel_name = {"kvj_r0_8_b3", "kvj_ptab"};
  img.kernel_src = {"// a\n", "// b\n"};
  img.variants.push_back({3u, {{'x'}, {}}});
  jit_save_plan("roundtrip", img);
  JitImage back;
  CHECK(jit_load_plan("roundtrip", &back) && same(back.plan, img.plan));
  // (the file lists the code objects of the two programs and of the one variant that ships)
  std::ifstream f(dir + "/plan-roundtrip.txt");
  int kernels = 0, cos = 0;
  for (std::string line; std::getline(f, line);) {
    kernels += line.rfind("kernel ", 0) == 0;
    cos += line.rfind("co kvj_", 0) == 0 && line.size() > 4 && line.substr(line.size() - 3) == ".co";
  }
  CHECK(kernels == 3 && cos == 3);
  const std::vector<JitKernelPlan> before = back.plan;
  put(dir + "/plan-badsum.txt", "kernel 0 8 6 2 3 3\nkernel 8 4 0 1 1 1\n");  // (blocks 3 != count 4)
  CHECK(!jit_load_plan("badsum", &back) && same(back.plan, before));
  put(dir + "/plan-noblocks.txt", "kernel 0 0 6\n");
  CHECK(!jit_load_plan("noblocks", &back) && same(back.plan, before));
  put(dir + "/plan-empty.txt", "");
  CHECK(!jit_load_plan("empty", &back) && same(back.plan, before));
  put(dir + "/plan-nokernels.txt", "co kvj_r0_8-0000000000000000.co\n");
  CHECK(!jit_load_plan("nokernels", &back) && same(back.plan, before));
  CHECK(!jit_load_plan("missing", &back) && same(back.plan, before));
}

// ---- the generator's programs (kvjitgen.cpp): helper records into kernel programs

// Every helper name (g_ / q_ / r_ + glob / atom / pred / blk / match / dleaf + _<n>) in `text`:
// a definition must be the first of its name and every use must follow its definition.
// `defs` receives the defined names in order, `uses` the number of uses.
bool helper_names_ok(const std::string& text, std::vector<std::string>* defs, size_t* uses) {
  static const char* kinds[] = {"glob_", "atom_", "pred_", "blk_", "match_", "dleaf_"};
  const std::string fn = "__device__ __forceinline__ bool ";
  auto ident = [](char c) { return isalnum((unsigned char)c) || c == '_'; };
  *uses = 0;
  defs->clear();
  for (size_t at = 0; at + 2 < text.size(); at++) {
    if ((text[at] != 'g' && text[at] != 'q' && text[at] != 'r') || text[at + 1] != '_' || (at && ident(text[at - 1]))) continue;
    size_t e = 0;
    for (const char* k : kinds)
      if (text.compare(at + 2, strlen(k), k) == 0) e = at + 2 + strlen(k);
    if (!e || e >= text.size() || !isdigit((unsigned char)text[e])) continue;
    while (e < text.size() && isdigit((unsigned char)text[e])) e++;
    const std::string name = text.substr(at, e - at);
    const bool known = std::find(defs->begin(), defs->end(), name) != defs->end();
    const bool def = at >= fn.size() && text.compare(at - fn.size(), fn.size(), fn) == 0;
    if (def ? known : !known) {
      fprintf(stderr, "%s of %s at offset %zu\n", def ? "second definition" : "use before the definition", name.c_str(), at);
      return false;
    }
    if (def) defs->push_back(name);
    else ++*uses;
    at = e - 1;
  }
  return true;
}

// A small hand-written policy set through compile_policies and jit_generate (no compile): two
// image globs of one structural form (a rule group), a quantity comparison, a name filter (its
// match function is called from the kernel), a pattern variable (the dynamic leaf's two functions
// are one record); two rules per kernel, so every program selects its own helpers.
void programs() {
  auto rule = [](const std::string& name, const std::string& match, const std::string& pattern) {
    return "{\"name\": \"" + name + "\", \"match\": {\"resources\": {" + match + "}}, \"validate\": {\"message\": \"m\", \"pattern\": " +
           pattern + "}}";
  };
  const std::string pod = "\"kinds\": [\"Pod\"]";
  const std::string policies =
      "[{\"apiVersion\": \"kyverno.io/v1\", \"kind\": \"ClusterPolicy\", \"metadata\": {\"name\": \"p\"}, "
      "\"spec\": {\"validationFailureAction\": \"Audit\", \"rules\": [" +
      rule("tag", pod, "{\"spec\": {\"containers\": [{\"image\": \"!*:latest\"}]}}") + ", " +
      rule("registry", pod, "{\"spec\": {\"containers\": [{\"image\": \"registry.example/*\"}]}}") + ", " +
      rule("memory", pod, "{\"spec\": {\"containers\": [{\"resources\": {\"limits\": {\"memory\": \"<=1Gi\"}}}]}}") + ", " +
      rule("named", pod + ", \"name\": \"pod-1*\"", "{\"metadata\": {\"name\": \"?*\"}}") + ", " +
      rule("label", pod, "{\"metadata\": {\"labels\": {\"app\": \"{{request.object.metadata.name}}\"}}}") + "]}}]";
  PolicySet ps;
  compile_policies(policies.data(), policies.size(), &ps, 0u);
  JitImage img;
  jit_generate(ps, 2, &img);
  CHECK(ps.rules.size() == 5 && img.kernel_src.size() == img.kernel_name.size() && img.kernel_src.size() >= 3);
  std::vector<std::string> all, defs;
  size_t uses = 0, fewer = 0, calling = 0;
  CHECK(helper_names_ok(img.source, &all, &uses) && uses > 0 && !all.empty());
  for (size_t i = 0; i < img.kernel_src.size(); i++) {
    const std::string& src = img.kernel_src[i];
    // the program ends with its kernel's own text: one kernel, of its name, and no helper after it
    const size_t k = src.find("extern \"C\" __global__");
    CHECK(k != std::string::npos && src.find("extern \"C\" __global__", k + 1) == std::string::npos);
    if (k == std::string::npos) continue;
    CHECK(src.find(" void " + img.kernel_name[i] + "(", k) != std::string::npos);
    CHECK(src.find("__device__ __forceinline__", k) == std::string::npos && src.compare(src.size() - 3, 3, "}\n\n") == 0);
    CHECK(img.source.find(src.substr(k)) != std::string::npos);
    // every helper it uses is defined in it, before the use
    CHECK(helper_names_ok(src, &defs, &uses));
    CHECK(defs.empty() == (uses == 0));  // (it takes helpers only if it uses some)
    calling += uses > 0;
    fewer += defs.size() < all.size();
    // (the dynamic leaf's wrapper and its evaluator travel together)
    const bool wrapper = std::find(defs.begin(), defs.end(), "g_dleaf_0") != defs.end();
    CHECK(wrapper == (src.find("__noinline__ bool kv_dleaf_impl") != std::string::npos));
  }
  // (kvj_ptab and the kernel of the name filter and the pattern variable call helpers; some program
  // leaves helpers out: the selection is per program)
  CHECK(calling >= 2 && fewer > 0);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: jitbuild_check <empty directory>\n");
    return 2;
  }
  verdict_domain();
  ladder();
  plan_file(argv[1]);
  programs();
  printf("{\"checks\": %d, \"failed\": %d}\n", checks, failed);
  return failed ? 1 : 0;
}
