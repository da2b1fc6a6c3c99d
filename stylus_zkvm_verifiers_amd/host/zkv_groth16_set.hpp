// C++ host wrapper of Groth16 key sets (include/zkv_groth16_set.h): `Groth16Verifier::verify_proof_with_key(vm_type, &vk, ...)`
// (/root/reference/contracts/src/common/groth16.rs:23-49) as a batch with a key per proof.  Library/runtime failures throw
// std::runtime_error; verdicts are never exceptions.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/zkv_groth16_set.h"

namespace zkv {

struct Groth16Key {
    std::vector<uint8_t> words;   // zkv_groth16_ctx_create's layout: 448 + 64 n_ic bytes
    size_t n_ic;
    int vm_type;                  // ZKV_VM_RISC0 / ZKV_VM_SP1
};

class Groth16VerifierSet {
public:
    explicit Groth16VerifierSet(const std::vector<Groth16Key>& keys, int device = 0) {
        std::vector<const uint8_t*> w; std::vector<size_t> n; std::vector<int> vm;
        for (const auto& k : keys) {
            if (k.words.size() != 448 + 64 * k.n_ic) throw std::invalid_argument("Groth16VerifierSet: key must be 448 + 64 n_ic bytes");
            w.push_back(k.words.data()); n.push_back(k.n_ic); vm.push_back(k.vm_type);
        }
        ctx_ = zkv_groth16_set_create(keys.size(), w.data(), n.data(), vm.data(), device);
        if (!ctx_) throw std::invalid_argument("zkv_groth16_set_create rejected the keys");
    }
    Groth16VerifierSet(Groth16VerifierSet&& o) noexcept : ctx_(o.ctx_) { o.ctx_ = nullptr; }
    Groth16VerifierSet(const Groth16VerifierSet&) = delete;
    Groth16VerifierSet& operator=(const Groth16VerifierSet&) = delete;
    ~Groth16VerifierSet() { if (ctx_) zkv_ctx_destroy(ctx_); }

    size_t size() const { return zkv_groth16_set_size(ctx_); }
    size_t signal_stride() const { return zkv_groth16_set_signal_stride(ctx_); }      // bytes per proof in `signals`

    // verified[i]: proof i (256 bytes) against key key[i] with the first n_ic - 1 words of signal row i; false for key[i] >= size()
    std::vector<bool> verify_batch(const std::vector<uint32_t>& key, const std::vector<uint8_t>& proofs, const std::vector<uint8_t>& signals) const {
        const size_t n = key.size();
        if (proofs.size() != 256 * n || signals.size() != signal_stride() * n) throw std::invalid_argument("Groth16VerifierSet::verify_batch: buffer sizes");
        std::vector<uint8_t> out(n ? n : 1);
        const int rc = zkv_groth16_set_verify_batch(ctx_, n, key.data(), proofs.data(), signals.data(), out.data());
        if (rc != ZKV_OK) throw std::runtime_error("zkv_groth16_set_verify_batch failed with ZKV error " + std::to_string(rc));
        return std::vector<bool>(out.begin(), out.begin() + n);
    }
    // Opt-in aggregate check (zkv_ctx_set_aggregate_check): sub_batch 0 = automatic size, 16 ... 256 fixed; seed32 = nullptr draws the secret
    // from the operating system.  enable = false switches it off.
    void set_aggregate_check(bool enable, const uint8_t* seed32 = nullptr, int sub_batch = 0) {
        const int rc = zkv_ctx_set_aggregate_check(ctx_, enable ? (sub_batch ? sub_batch : 1) : 0, seed32);
        if (rc != ZKV_OK) throw std::invalid_argument("zkv_ctx_set_aggregate_check failed with ZKV error " + std::to_string(rc));
    }
    // {sub-batches checked in aggregate, sub-batches that failed and were verified proof by proof}
    std::vector<uint64_t> aggregate_counters() const {
        uint64_t v[2] = {0, 0};
        const int rc = zkv_ctx_aggregate_counters(ctx_, v);
        if (rc != ZKV_OK) throw std::runtime_error("zkv_ctx_aggregate_counters failed with ZKV error " + std::to_string(rc));
        return {v[0], v[1]};
    }
    zkv_ctx* handle() const { return ctx_; }

private:
    zkv_ctx* ctx_ = nullptr;
};

}  // namespace zkv
