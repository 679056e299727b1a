// The caller's side of the two rate-matching lines of ITTC/main.cpp (196, 204), for
// tests/test_ratematch_host.py: the declarations are ITTC/main.h:23-24 word for word, so the link
// resolves whatever names the compiler gives them against libturbo_logmap_compat.so.
//   ratematch_driver K E in.bin e.bin back.bin
// in.bin: int32 [3K+12] -> e.bin: int32 [E] = rate_match(in); back.bin: double [3K+12] =
// de_rate_match of e as doubles.
#include <cstdio>
#include <cstdlib>
#include <vector>

int source_length = 40;   // the globals the compat layer reads (ITTC/main.h:6-11)
int f1 = 3, f2 = 10;

void rate_match(int* input,int in_len,int*output,int out_len);
void de_rate_match(double*input,double*output,int in_len,int out_len);

int main(int argc, char** argv)
{
    if (argc != 6) return 2;
    const int K = std::atoi(argv[1]), E = std::atoi(argv[2]), n = 3 * K + 12;
    std::vector<int> in(n), e(E);
    FILE* f = std::fopen(argv[3], "rb");
    if (!f || std::fread(in.data(), sizeof(int), n, f) != (size_t)n) return 3;
    std::fclose(f);
    rate_match(in.data(), n, e.data(), E);
    std::vector<double> soft(e.begin(), e.end()), back(n, -1.0);
    de_rate_match(soft.data(), back.data(), E, n);
    f = std::fopen(argv[4], "wb");
    if (!f || std::fwrite(e.data(), sizeof(int), E, f) != (size_t)E) return 4;
    std::fclose(f);
    f = std::fopen(argv[5], "wb");
    if (!f || std::fwrite(back.data(), sizeof(double), n, f) != (size_t)n) return 5;
    std::fclose(f);
    return 0;
}
