// Replays a recording of conv calls (tools/record_conv_routes.py, tests/fixtures/conv_dma_routes.txt) through
// the LDS-DMA planner (csrc/conv_dma_plan.h) on the CPU: every row the GPU routed to this family (dma / kw3 /
// kw3p / group) must get the same route from dma_plan() at the recorded CU count and knobs. Rows of the
// other kernels (igemm, halo, halo-stream, pw, ...) are the only ones skipped.
//
// From each row it rebuilds the planner's scalar inputs the way bindings.cpp:conv() does: the geometry, the
// null / non-null tests of the optional tensors (any non-null address stands for "present"), vec_epi and
// pool_t from the two alignment rules, the unpool / ReLU-copy pre-passes (x_ld = C afterwards).
//
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__=1 -I<rocm>/include -I<csrc> conv_dma_plan_check.cpp && ./a.out <fixture>
#include "conv_dma_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <set>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

namespace {

std::vector<std::string> split(const std::string& s, char sep) {
  std::vector<std::string> out;
  std::stringstream ss(s);
  for (std::string t; std::getline(ss, t, sep);) out.push_back(t);
  return out;
}

struct TensorInfo {
  bool present = false;
  long long align = 0, ld = 0, elems = 0;  // pointer mod 16, row stride, storage elements past the pointer
};
TensorInfo tensor(const std::string& v) {
  TensorInfo t;
  if (v == "-") return t;
  const auto f = split(v, ',');
  if (f.size() != 3) throw std::runtime_error("bad tensor field " + v);
  t.present = true;
  t.align = std::atoll(f[0].c_str());
  t.ld = std::atoll(f[1].c_str());
  t.elems = std::atoll(f[2].c_str());
  return t;
}

int fail(int line, const std::string& why) {
  std::fprintf(stderr, "line %d: %s\n", line, why.c_str());
  return 1;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return fail(0, "usage: conv_dma_plan_check <recording>");
  std::ifstream in(argv[1]);
  if (!in) return fail(0, std::string("cannot open ") + argv[1]);
  static char present;  // any non-null address: the planner only tests these pointers for null
  int lineno = 0, checked = 0, skipped = 0, bad = 0;
  std::set<std::string> forms;
  for (std::string line; std::getline(in, line);) {
    ++lineno;
    if (line.empty() || line[0] == '#') continue;
    const size_t bar = line.find(" | ");
    if (bar == std::string::npos) return fail(lineno, "no route");
    const std::string want = line.substr(bar + 3);
    std::map<std::string, std::string> kv;
    for (const auto& tok : split(line.substr(0, bar), ' ')) {
      const size_t eq = tok.find('=');
      if (eq != std::string::npos) kv[tok.substr(0, eq)] = tok.substr(eq + 1);
    }
    for (const char* key : {"g", "amode", "epi", "impl", "dt", "has", "relu_cols", "split_col", "ucode_div", "out", "res",
                            "emask", "out_code", "cus", "knobs"})
      if (!kv.count(key)) return fail(lineno, std::string("missing field ") + key);
    // the route without its pre-pass prefixes
    std::string core = want;
    for (const char* pre : {"unpool2x2 > ", "relu_copy > "})
      if (core.rfind(pre, 0) == 0) core = core.substr(std::strlen(pre));
    const bool group = core.rfind("group ", 0) == 0;
    if (!(core.rfind("dma ", 0) == 0 || core.rfind("kw3 ", 0) == 0 || core.rfind("kw3p ", 0) == 0 || group)) {
      ++skipped;
      continue;
    }
    const auto g = split(kv["g"], ',');
    if (g.size() != 23) return fail(lineno, "geometry must have 23 entries");
    auto gi = [&](int i) { return std::atoll(g[i].c_str()); };
    dv::ConvArgs a{};
    a.N = (int)gi(0); a.H = (int)gi(1); a.W = (int)gi(2); a.C = (int)gi(3);
    a.OH = (int)gi(4); a.OW = (int)gi(5); a.OC = (int)gi(6); a.OCpad = (int)gi(7);
    a.KH = (int)gi(8); a.KW = (int)gi(9); a.stride = (int)gi(10); a.pad_h = (int)gi(11); a.pad_w = (int)gi(12);
    a.K = (int)gi(13); a.Kpad = (int)gi(14); a.M = (int)gi(15);
    a.relu = (int)gi(16); a.relu_in = (int)gi(17); a.accumulate = (int)gi(18);
    a.code_div = (int)gi(19); a.x_ld = gi(20); a.mask_ld = gi(21); a.out_ld = gi(22);
    a.relu_cols = std::atoi(kv["relu_cols"].c_str());
    a.dtype = kv["dt"] == "f16" ? dv::DT_F16 : dv::DT_BF16;
    int amode = std::atoi(kv["amode"].c_str());
    const int epi = std::atoi(kv["epi"].c_str());
    std::set<std::string> has;
    for (const auto& h : split(kv["has"], ',')) has.insert(h);
    const TensorInfo out = tensor(kv["out"]), res = tensor(kv["res"]), emask = tensor(kv["emask"]),
                     out_code = tensor(kv["out_code"]);
    const void* some = &present;
    a.out_elems = out.elems;
    if (has.count("mask")) a.mask = static_cast<const uint16_t*>(some);
    if (res.present) {
      a.res = static_cast<const uint16_t*>(some);
      a.res_ld = res.ld;
    }
    if (emask.present) {
      a.emask = static_cast<const uint16_t*>(some);
      a.emask_ld = emask.ld;
    }
    if (has.count("ucode")) {
      a.ucode = static_cast<const uint8_t*>(some);
      a.ucode_div = std::atoi(kv["ucode_div"].c_str());
    }
    if (has.count("out2")) {
      a.out2 = &present;
      a.split_col = std::atoi(kv["split_col"].c_str());
    }
    if (has.count("w_kw3")) a.wp = static_cast<const uint16_t*>(some);
    // the two alignment rules of bindings.cpp
    auto al = [](const TensorInfo& t) { return t.align % 16 == 0 && t.ld % 8 == 0; };
    a.vec_epi = epi == dv::CONV_E_BF16 && out.align % 16 == 0 && a.out_ld % 8 == 0 && (!res.present || al(res)) &&
                (!emask.present || al(emask));
    if (epi == dv::CONV_E_POOL)
      a.pool_t = a.OC % 4 == 0 && a.out_ld % 4 == 0 && out.align % 8 == 0 && out_code.present && out_code.align % 4 == 0;
    // the pre-passes: an unpool input is materialized, a ReLU'd input copied, both channel-dense
    std::string prefix;
    if (amode == dv::CONV_A_UNPOOL) {
      prefix += "unpool2x2 > ";
      amode = dv::CONV_A_FWD;
      a.x_ld = a.C;
      a.relu_in = 0;
    }
    if (a.relu_in) {
      prefix += "relu_copy > ";
      a.x_ld = a.C;
      if (a.mask) a.mask_ld = a.C;
      a.relu_in = 0;
    }
    dv::DmaKnobs k;  // set from the row, never from the environment
    if (kv["knobs"] != "-") {
      for (const auto& item : split(kv["knobs"], ',')) {
        const size_t eq = item.find('=');
        const std::string name = item.substr(0, eq), val = eq == std::string::npos ? "" : item.substr(eq + 1);
        if (name == "DV_KW3") k.kw3 = std::atoi(val.c_str());
        else if (name == "DV_KW3_VAR") k.kw3_var = std::atoi(val.c_str());
        else if (name == "DV_KW3_TILE") k.kw3_tile_512 = val == "512x128";
        else if (name == "DV_KW3_SK") k.kw3_sk_all = val == "all";
        else if (name == "DV_NO_KW3_SK") k.no_kw3_sk = true;
        else if (name == "DV_KW3P_EPI") k.kw3p_epi_reg = val == "reg";
        else if (name == "DV_KW3P_UNP_NT") k.kw3p_unp_nt = val != "0";
        else if (name == "DV_NO_KW3P_UNPOOL") k.no_kw3p_unpool = true;
        else if (name == "DV_KW3P_NO_PRE") k.kw3p_no_pre = true;
        else if (name == "cfg") k.cfg = std::atoi(val.c_str());
        else if (name == "ks") k.ks = std::atoi(val.c_str());
        else return fail(lineno, "unknown knob " + name);
      }
    }
    const dv::DmaPlan p = dv::dma_plan(a, amode, epi, std::atoi(kv["cus"].c_str()), k);
    std::string got;
    if (group) {  // recorded inside an open conv group: the binding reports the plan's group config
      const int impl = std::atoi(kv["impl"].c_str());
      const bool recordable = (impl == 0 || impl == 2) && !a.mask && prefix.empty() && !a.ucode && !a.out2 && !has.count("stats");
      dv::ConvRoute r{};
      r.kind = recordable && p.group_cfg != 0 ? dv::CR_GROUP : dv::CR_NONE;
      r.cfg = p.group_cfg;
      got = dv::route_str(r);
    } else if (p.status != 0) {
      got = "declined " + std::to_string(p.status);
    } else {
      got = prefix + dv::route_str(dv::plan_route(p));
    }
    ++checked;
    // the form of the route: its words without the numbers that follow the CU count
    forms.insert(core.substr(0, core.find(" m_base=")));
    if (got != want) {
      ++bad;
      std::fprintf(stderr, "line %d: planner says '%s', recorded '%s'\n  %s\n", lineno, got.c_str(), want.c_str(), line.c_str());
    }
  }
  // every form the recording must hold (the issue's list), so a thinned fixture cannot pass quietly
  auto any = [&](const char* pre, const char* word) {
    for (const auto& f : forms)
      if (f.rfind(pre, 0) == 0 && (!*word || (" " + f + " ").find(std::string(" ") + word + " ") != std::string::npos)) return true;
    return false;
  };
  auto any_ks = [&] {
    for (const auto& f : forms) {
      const size_t i = f.find(" ks");
      if (f.rfind("dma ", 0) == 0 && i != std::string::npos && std::atoi(f.c_str() + i + 3) > 1) return true;
    }
    return false;
  };
  const struct { const char* name; bool ok; } need[] = {
      {"dma ks1", any("dma ", "ks1")}, {"dma ks>1", any_ks()}, {"dma mask", any("dma ", "mask")},
      {"dma pool_t", any("dma ", "pool_t")}, {"kw3", any("kw3 ", "")}, {"kw3p lds", any("kw3p ", "lds")},
      {"kw3p reg", any("kw3p ", "reg")}, {"kw3p unpool", any("kw3p ", "unpool")}, {"kw3p sk", any("kw3p ", "sk")},
      {"kw3p tail", any("kw3p ", "tail")}, {"group cfg8", any("group cfg8", "")}, {"group cfg3", any("group cfg3", "")}};
  for (const auto& n : need)
    if (!n.ok) {
      ++bad;
      std::fprintf(stderr, "the recording holds no '%s' row\n", n.name);
    }
  std::printf("checked=%d skipped=%d forms=%d mismatches=%d\n", checked, skipped, (int)forms.size(), bad);
  return bad == 0 && checked > 0 ? 0 : 1;
}
