// C++ host wrapper of Groth16 key sets (include/zkv_groth16_set.h): `Groth16Verifier::verify_proof_with_key(vm_type, &vk, ...)`
// (/root/reference/contracts/src/common/groth16.rs:23-49) as a batch with a key per proof.  Library/runtime failures throw
// std::runtime_error; verdicts are never exceptions.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/zkv_groth16_set.h"
#include "../../include/zkv_groth16_set_wire.h"

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

protected:
    explicit Groth16VerifierSet(zkv_ctx* adopted) : ctx_(adopted) {}
    zkv_ctx* ctx_ = nullptr;
};

// A key set whose keys are deployed verifier contracts (include/zkv_groth16_set_wire.h; parity unpinned: the reference holds no generic
// contract shell): Groth16VerifierSet plus eth_call batches of raw `verifyProof` calldata, each request addressed to a contract.
struct Groth16Contract {
    Groth16Key key;
    uint8_t address[20];
    int form;                     // ZKV_G16_FORM_SNARKJS / ZKV_G16_FORM_GNARK
};

struct EthCallResults {
    std::vector<uint8_t> reverted, status;
    std::vector<std::vector<uint8_t>> returndata;
};

class Groth16DeployedSet : public Groth16VerifierSet {
public:
    explicit Groth16DeployedSet(const std::vector<Groth16Contract>& contracts, int device = 0) : Groth16VerifierSet(create(contracts, device)) {}

    // the 4-byte selector of a form's verifyProof with n_signals public signals
    static std::vector<uint8_t> selector(int form, size_t n_signals) {
        std::vector<uint8_t> out(4);
        if (zkv_groth16_set_call_selector(form, n_signals, out.data()) != ZKV_OK) throw std::invalid_argument("Groth16DeployedSet::selector: form or signal count");
        return out;
    }
    // canonical calldata of verifyProof: selector, the 256 proof bytes (the precompiles' word order), the 32-byte signals
    static std::vector<uint8_t> encode_call(int form, const std::vector<uint8_t>& proof_words, const std::vector<uint8_t>& signals) {
        if (proof_words.size() != 256 || signals.size() % 32) throw std::invalid_argument("Groth16DeployedSet::encode_call: a proof is 256 bytes and a signal 32");
        std::vector<uint8_t> out = selector(form, signals.size() / 32);
        out.insert(out.end(), proof_words.begin(), proof_words.end());
        out.insert(out.end(), signals.begin(), signals.end());
        return out;
    }
    // request i: calls[i] to the contract at to[20 i ..]
    EthCallResults eth_call_batch(const std::vector<uint8_t>& to, const std::vector<std::vector<uint8_t>>& calls) const {
        const size_t n = calls.size();
        if (to.size() != 20 * n) throw std::invalid_argument("Groth16DeployedSet::eth_call_batch: one 20-byte address per request");
        std::vector<uint64_t> off(n + 1, 0);
        std::vector<uint8_t> blob;
        for (size_t i = 0; i < n; i++) { blob.insert(blob.end(), calls[i].begin(), calls[i].end()); off[i + 1] = blob.size(); }
        blob.push_back(0);
        EthCallResults r;
        r.reverted.assign(n ? n : 1, 0); r.status.assign(n ? n : 1, 0);
        std::vector<uint8_t> data((n ? n : 1) * ZKV_RETURNDATA_STRIDE);
        std::vector<uint32_t> len(n ? n : 1, 0);
        const int rc = zkv_groth16_set_eth_call_batch(ctx_, n, to.data(), blob.data(), off.data(), r.reverted.data(), data.data(), len.data(), r.status.data());
        if (rc != ZKV_OK) throw std::runtime_error("zkv_groth16_set_eth_call_batch failed with ZKV error " + std::to_string(rc));
        r.reverted.resize(n); r.status.resize(n);
        for (size_t i = 0; i < n; i++) r.returndata.emplace_back(data.begin() + i * ZKV_RETURNDATA_STRIDE, data.begin() + i * ZKV_RETURNDATA_STRIDE + len[i]);
        return r;
    }
    // every buffer in device memory, enqueued on `stream` (nullptr: the context's); d_key may be nullptr
    void eth_call_batch_dev(size_t n, const uint8_t* d_to, const uint8_t* d_calldata, const uint64_t* d_calldata_off, uint64_t calldata_bytes, uint8_t* d_status,
                            uint32_t* d_key = nullptr, void* stream = nullptr) const {
        const int rc = zkv_groth16_set_eth_call_batch_dev(ctx_, n, d_to, d_calldata, d_calldata_off, calldata_bytes, d_status, d_key, stream);
        if (rc != ZKV_OK) throw std::runtime_error("zkv_groth16_set_eth_call_batch_dev failed with ZKV error " + std::to_string(rc));
    }
    // {placed, no contract, bad calldata, signal not in field} of the most recent eth_call batch
    std::vector<uint64_t> last_call_counts() const {
        uint64_t v[4] = {0, 0, 0, 0};
        const int rc = zkv_groth16_set_last_call_counts(ctx_, v);
        if (rc != ZKV_OK) throw std::runtime_error("zkv_groth16_set_last_call_counts failed with ZKV error " + std::to_string(rc));
        return {v[0], v[1], v[2], v[3]};
    }

private:
    static zkv_ctx* create(const std::vector<Groth16Contract>& contracts, int device) {
        std::vector<const uint8_t*> w; std::vector<size_t> n; std::vector<int> vm; std::vector<uint8_t> addr, form;
        for (const auto& c : contracts) {
            if (c.key.words.size() != 448 + 64 * c.key.n_ic) throw std::invalid_argument("Groth16DeployedSet: key must be 448 + 64 n_ic bytes");
            w.push_back(c.key.words.data()); n.push_back(c.key.n_ic); vm.push_back(c.key.vm_type);
            addr.insert(addr.end(), c.address, c.address + 20); form.push_back((uint8_t)c.form);
        }
        zkv_ctx* ctx = zkv_groth16_set_create_deployed(contracts.size(), w.data(), n.data(), vm.data(), addr.data(), form.data(), device);
        if (!ctx) throw std::invalid_argument("zkv_groth16_set_create_deployed rejected the contracts");
        return ctx;
    }
};

}  // namespace zkv
