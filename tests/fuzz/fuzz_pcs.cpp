// Fuzz driver for the opening parser of the polynomial commitment: hg_pcs_verify and hg_claims_verify read untrusted bytes. Built
// with -fsanitize=fuzzer,address,undefined against build/asan/libhypergreco.so like fuzz_host.cpp; host only, no context anywhere.
// Targets, selected by HG_FUZZ_TARGET:
//   pcs      the bytes are an opening of three claims (Q = 3) on two fixed tables (6 and 2 variables, c = 2): hg_pcs_verify must
//            accept or reject with a reason; the honest opening itself must be accepted
//   pcsargs  eight leading bytes choose log2_row, n_queries, the claim count, the claims' table indices and the table count (out of
//            range values included), the rest is the opening: every -1 path and the length arithmetic
//   claims   the bytes are an opening (Q = 4) of five claims on the secret inputs of the n=1024 reference witness: hg_claims_verify
// Claims sit at Boolean points, where the value is a table word, so the driver needs no evaluator to build honest ones.
// HG_FUZZ_SEEDS=<dir>: the honest opening of the target is written there as a seed before the run starts.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/hg.h"

static int target = 0;
static const uint64_t GL_P = 0xFFFFFFFF00000001ull;

// ---- generic layer: two tables
static const uint32_t NVARS[3] = {6, 2, 3};
static std::vector<uint64_t> T0(64), T1(4);
static uint8_t ROOT[32];
static uint32_t TABLE[4] = {0, 1, 0, 1};
static std::vector<uint64_t> POINTS, VALUES;
static std::vector<uint8_t> HONEST;
static const std::vector<uint64_t> ARGPOINTS(4 * 6 * 2, 1);   // pcsargs: room for four claims on the widest table

// ---- the secret inputs of the reference witness
static hg_params PR;
static uint8_t SROOT[32];
static std::vector<hg_input_claim> CLAIMS;
static std::vector<uint64_t> CPOINTS;
static std::vector<uint8_t> CHONEST;

static void die(const char* what) { fprintf(stderr, "%s: %s\n", what, hg_last_error()); abort(); }
static void write_seed(const char* name, const std::vector<uint8_t>& bytes) {
    const char* dir = getenv("HG_FUZZ_SEEDS");
    if (!dir) return;
    FILE* f = fopen((std::string(dir) + "/" + name).c_str(), "wb");
    if (!f) return;
    fwrite(bytes.data(), 1, bytes.size(), f);
    fclose(f);
}
static void boolean_point(std::vector<uint64_t>& out, size_t index, size_t nvars) {
    for (size_t b = 0; b < nvars; b++) { out.push_back((index >> b) & 1); out.push_back(0); }
}

extern "C" int LLVMFuzzerInitialize(int*, char***) {
    const char* t = getenv("HG_FUZZ_TARGET");
    target = !t || !strcmp(t, "pcs") ? 0 : (!strcmp(t, "pcsargs") ? 1 : 2);
    if (target < 2) {
        uint64_t x = 0x9e3779b97f4a7c15ull;
        for (auto* tab : {&T0, &T1})
            for (auto& v : *tab) { x = x * 6364136223846793005ull + 1442695040888963407ull; v = x % GL_P; }
        T0[5] = GL_P - 1; T0[6] = 0;
        const uint64_t* tabs[2] = {T0.data(), T1.data()};
        void* cm = nullptr;
        if (hg_pcs_commit(nullptr, tabs, NVARS, 2, 2, &cm, ROOT) != 0) die("commit");
        const size_t at[4] = {5, 3, 62, 0};
        for (int i = 0; i < 4; i++) {
            boolean_point(POINTS, at[i], NVARS[TABLE[i]]);
            VALUES.push_back(TABLE[i] ? T1[at[i]] : T0[at[i]]);
            VALUES.push_back(0);
        }
        HONEST.resize(1 << 16);
        size_t len = 0;
        if (hg_pcs_open(nullptr, cm, TABLE, POINTS.data(), VALUES.data(), 3, 3, HONEST.data(), HONEST.size(), &len) != 0) die("open");
        HONEST.resize(len);
        hg_pcs_free(cm);
        if (hg_pcs_verify(ROOT, NVARS, 2, 2, TABLE, POINTS.data(), VALUES.data(), 3, 3, HONEST.data(), HONEST.size()) != 0) die("the honest opening");
        std::vector<uint8_t> seed = HONEST;
        if (target == 1) { const uint8_t head[8] = {2, 3, 3, 0, 1, 0, 1, 2}; seed.insert(seed.begin(), head, head + 8); }
        write_seed("honest", seed);
        return 0;
    }
    const char* root = getenv("HG_FUZZ_ROOT");
    const std::string gold = std::string(root ? root : ".") + "/tests/golden/";
    hg_witness* w = nullptr;
    if (hg_params_builtin(1024, 1, &PR) != 0) die("params");
    if (hg_witness_from_json(&PR, (gold + "sk_enc_1024_1x27_65537.json").c_str(), &w) != 0) die("witness");
    void* cm = nullptr;
    if (hg_secrets_commit(nullptr, &PR, w, 0, &cm, SROOT) != 0) die("secrets commit");
    // one claim per secret input (k = 1: inputs 0, 1, 2, 4, 5; witness tables 0 s, 1 e, 2 k1, 4 r1is, 5 r2is)
    const uint32_t input[5] = {0, 1, 2, 4, 5}, nv[5] = {11, 11, 11, 11, 10};
    const int which[5] = {0, 1, 2, 4, 5};
    const size_t at[5] = {1000, 1500, 2046, 1200, 77};
    for (int i = 0; i < 5; i++) {
        std::vector<uint64_t> tab((size_t)1 << nv[i]);
        if (hg_witness_get(w, which[i], tab.data(), tab.size()) != (int64_t)tab.size()) die("witness table");
        hg_input_claim c;
        c.input = input[i]; c.nvars = nv[i]; c.point_off = CPOINTS.size() / 2;
        c.value[0] = tab[at[i]]; c.value[1] = 0;
        boolean_point(CPOINTS, at[i], nv[i]);
        CLAIMS.push_back(c);
    }
    CHONEST.resize(1 << 20);
    size_t len = 0;
    if (hg_claims_open(nullptr, &PR, cm, CLAIMS.data(), CLAIMS.size(), CPOINTS.data(), 4, CHONEST.data(), CHONEST.size(), &len) != 0) die("claims open");
    CHONEST.resize(len);
    hg_pcs_free(cm);
    hg_witness_free(w);
    if (hg_claims_verify(&PR, SROOT, 0, CLAIMS.data(), CLAIMS.size(), CPOINTS.data(), 4, CHONEST.data(), CHONEST.size()) != 0) die("the honest opening");
    write_seed("honest", CHONEST);
    return 0;
}

static void settled(int rc) {
    if (rc < -1 || rc > 1) abort();
    if (rc != 0 && (!hg_last_error() || !*hg_last_error())) abort();   // a rejection or an error without a reason is a bug too
}

extern "C" int LLVMFuzzerTestOneInput(const uint8_t* data, size_t size) {
    if (target == 0) {
        const int rc = hg_pcs_verify(ROOT, NVARS, 2, 2, TABLE, POINTS.data(), VALUES.data(), 3, 3, data, size);
        settled(rc);
        if (rc != 0 && size == HONEST.size() && !memcmp(data, HONEST.data(), size)) abort();
    } else if (target == 1) {
        if (size < 8) return 0;
        uint32_t table[4];
        for (int i = 0; i < 4; i++) table[i] = data[3 + i] % 4;
        settled(hg_pcs_verify(ROOT, NVARS, data[7] % 4, data[0] % 8, table, ARGPOINTS.data(), VALUES.data(), data[2] % 5, data[1] % 8, data + 8, size - 8));
    } else {
        settled(hg_claims_verify(&PR, SROOT, 0, CLAIMS.data(), CLAIMS.size(), CPOINTS.data(), 4, data, size));
    }
    return 0;
}
