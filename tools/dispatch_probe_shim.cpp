// The HIP entry points libptb_hip.so imports, defined so that a launch only records which kernel it names (tools/dispatch_probe.py): no GPU.
#include <cstdio>
#include <cstddef>
#include <map>
#include <string>
struct D3 { unsigned x, y, z; };
static std::map<const void*, std::string>& names() { static std::map<const void*, std::string> m; return m; }
static thread_local struct { D3 g, b; size_t sh; void* st; } cfg;
static FILE* g_log = nullptr;
extern "C" {
void ptb_shim_open(const char* path) { g_log = fopen(path, "w"); }
void ptb_shim_mark(const char* text) { fprintf(g_log, "# %s\n", text); }
void ptb_shim_close() { fclose(g_log); g_log = nullptr; }
int __hipPushCallConfiguration(D3 g, D3 b, size_t sh, void* st) { cfg.g = g; cfg.b = b; cfg.sh = sh; cfg.st = st; return 0; }
int __hipPopCallConfiguration(D3* g, D3* b, size_t* sh, void** st) { *g = cfg.g; *b = cfg.b; *sh = cfg.sh; *st = cfg.st; return 0; }
void** __hipRegisterFatBinary(const void*) { static void* h; return &h; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host, char*, const char* dev, unsigned, void*, void*, void*, void*, int*) { names()[host] = dev; }
int hipGetLastError() { return 0; }
const char* hipGetErrorString(int) { return ""; }
int hipMemsetAsync(void*, int, size_t, void*) { return 0; }
int hipMemcpyAsync(void*, const void*, size_t, int, void*) { return 0; }
int hipEventRecord(void*, void*) { return 0; }
int hipLaunchKernel(const void* f, D3 g, D3 b, void**, size_t sh, void*) {
    auto it = names().find(f);
    if (g_log) fprintf(g_log, "%s grid %u,%u,%u block %u,%u,%u lds %zu\n", it == names().end() ? "?" : it->second.c_str(), g.x, g.y, g.z, b.x, b.y, b.z, sh);
    return 0;
}
}
