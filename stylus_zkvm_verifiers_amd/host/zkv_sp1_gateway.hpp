// C++ host wrapper of the SP1 gateway (include/zkv_sp1_gateway.h): `ISp1Verifier::verify_proof` with the verifier chosen per proof by
// the first 4 bytes of `proof_bytes`, as SP1's on-chain gateway does.  Library/runtime failures throw std::runtime_error; statuses
// (ZKV_STATUS_*, ZKV_STATUS_ROUTE_NOT_FOUND) are never exceptions.  Parity unpinned: the reference holds no gateway and no PLONK code.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/zkv_sp1_gateway.h"
#include "../../include/zkv_sp1_gateway_wire.h"
#include "../../include/zkv_sp1_gateway_keys.h"

namespace zkv {

struct Sp1PlonkRoute {
    std::vector<uint8_t> vk;              // zkv_sp1_plonk_ctx_create's layout
    std::vector<uint8_t> verifier_hash;   // 32 bytes; its first four are the route's selector
};

struct Sp1Groth16Route {
    std::vector<uint8_t> vk_words;        // ZKV_SP1_GROTH16_KEY_BYTES: zkv_groth16_ctx_create's layout with n_ic = 3, SP1's sign convention
    std::vector<uint8_t> verifier_hash;   // 32 bytes; its first four are the route's selector
};

class Sp1Gateway {
public:
    // Route order: the built-in Groth16 route, the keyed Groth16 routes, the PLONK routes (include/zkv_sp1_gateway_keys.h)
    Sp1Gateway(bool groth16, const std::vector<Sp1Groth16Route>& groth16_keys, const std::vector<Sp1PlonkRoute>& plonk, int device = 0) {
        std::vector<const uint8_t*> key, vk; std::vector<size_t> len; std::vector<uint8_t> key_hashes, hashes;
        for (const auto& r : groth16_keys) {
            if (r.vk_words.size() != ZKV_SP1_GROTH16_KEY_BYTES) throw std::invalid_argument("Sp1Gateway: a keyed Groth16 route takes a key with n_ic = 3");
            if (r.verifier_hash.size() != 32) throw std::invalid_argument("Sp1Gateway: verifier_hash must be 32 bytes");
            key.push_back(r.vk_words.data()); key_hashes.insert(key_hashes.end(), r.verifier_hash.begin(), r.verifier_hash.end());
        }
        for (const auto& r : plonk) {
            if (r.verifier_hash.size() != 32) throw std::invalid_argument("Sp1Gateway: verifier_hash must be 32 bytes");
            vk.push_back(r.vk.data()); len.push_back(r.vk.size()); hashes.insert(hashes.end(), r.verifier_hash.begin(), r.verifier_hash.end());
        }
        ctx_ = zkv_sp1_gateway_create_keyed(groth16 ? 1 : 0, groth16_keys.size(), key.data(), key_hashes.data(), plonk.size(), vk.data(), len.data(),
                                            hashes.data(), device);
        if (!ctx_) throw std::invalid_argument("zkv_sp1_gateway_create_keyed rejected the routes");
    }
    Sp1Gateway(bool groth16, const std::vector<Sp1PlonkRoute>& plonk, int device = 0) {
        std::vector<const uint8_t*> vk; std::vector<size_t> len; std::vector<uint8_t> hashes;
        for (const auto& r : plonk) {
            if (r.verifier_hash.size() != 32) throw std::invalid_argument("Sp1Gateway: verifier_hash must be 32 bytes");
            vk.push_back(r.vk.data()); len.push_back(r.vk.size()); hashes.insert(hashes.end(), r.verifier_hash.begin(), r.verifier_hash.end());
        }
        ctx_ = zkv_sp1_gateway_create(groth16 ? 1 : 0, plonk.size(), vk.data(), len.data(), hashes.data(), device);
        if (!ctx_) throw std::invalid_argument("zkv_sp1_gateway_create rejected the routes");
    }
    Sp1Gateway(Sp1Gateway&& o) noexcept : ctx_(o.ctx_) { o.ctx_ = nullptr; }
    Sp1Gateway(const Sp1Gateway&) = delete;
    Sp1Gateway& operator=(const Sp1Gateway&) = delete;
    ~Sp1Gateway() { if (ctx_) zkv_ctx_destroy(ctx_); }

    size_t route_count() const { return zkv_sp1_gateway_route_count(ctx_); }
    std::vector<uint8_t> route_verifier_hash(size_t r) const {
        std::vector<uint8_t> out(32);
        if (zkv_sp1_gateway_route_verifier_hash(ctx_, r, out.data()) != ZKV_OK) throw std::invalid_argument("Sp1Gateway::route_verifier_hash: no such route");
        return out;
    }

    // status[i] / recv[4 i .. 4 i + 4) of proof i (ragged host buffers, as zkv_sp1_verify_batch)
    void verify_batch(const std::vector<uint8_t>& vkeys, const std::vector<uint8_t>& pv_blob, const std::vector<uint64_t>& pv_off,
                      const std::vector<uint8_t>& proof_blob, const std::vector<uint64_t>& proof_off, std::vector<uint8_t>& status,
                      std::vector<uint8_t>& recv) const {
        const size_t n = proof_off.empty() ? 0 : proof_off.size() - 1;
        if (vkeys.size() != 32 * n || pv_off.size() != proof_off.size()) throw std::invalid_argument("Sp1Gateway::verify_batch: buffer sizes");
        status.assign(n, 0); recv.assign(4 * n, 0);
        const uint8_t zero = 0;
        const int rc = zkv_sp1_gateway_verify_batch(ctx_, n, vkeys.data(), pv_blob.empty() ? &zero : pv_blob.data(), pv_off.data(),
                                                    proof_blob.empty() ? &zero : proof_blob.data(), proof_off.data(), status.data(), recv.data());
        if (rc != ZKV_OK) throw std::runtime_error("zkv_sp1_gateway_verify_batch failed with ZKV error " + std::to_string(rc));
    }
    // {proofs per route..., not found, shorter than 4 bytes} of the most recent call
    std::vector<uint64_t> last_route_counts() const {
        std::vector<uint64_t> out(route_count() + 2);
        const int rc = zkv_sp1_gateway_last_route_counts(ctx_, out.data());
        if (rc != ZKV_OK) throw std::runtime_error("zkv_sp1_gateway_last_route_counts failed with ZKV error " + std::to_string(rc));
        return out;
    }
    // eth_call batches (include/zkv_sp1_gateway_wire.h): raw verifyProof calldata, either form, Groth16 and PLONK proofs mixed.
    // Canonical calldata of one call; form = ZKV_CALLDATA_FORM_UINT8_ARRAY or ZKV_CALLDATA_FORM_BYTES.
    static std::vector<uint8_t> encode_verify_proof_call(int form, const uint8_t vkey[32], const std::vector<uint8_t>& pv, const std::vector<uint8_t>& proof) {
        const size_t n = zkv_sp1_gateway_encode_verify_proof_call(form, vkey, pv.data(), pv.size(), proof.data(), proof.size(), nullptr, 0);
        if (!n) throw std::invalid_argument("Sp1Gateway::encode_verify_proof_call: no such calldata form");
        std::vector<uint8_t> out(n);
        zkv_sp1_gateway_encode_verify_proof_call(form, vkey, pv.data(), pv.size(), proof.data(), proof.size(), out.data(), n);
        return out;
    }
    struct EthCallResult { std::vector<uint8_t> reverted, returndata, status; std::vector<uint32_t> returndata_len; };   // returndata: n x ZKV_RETURNDATA_STRIDE
    EthCallResult eth_call_batch(const std::vector<uint8_t>& calldata_blob, const std::vector<uint64_t>& calldata_off) const {
        const size_t n = calldata_off.empty() ? 0 : calldata_off.size() - 1;
        EthCallResult r;
        r.reverted.assign(n, 0); r.status.assign(n, 0); r.returndata_len.assign(n, 0); r.returndata.assign(n * ZKV_RETURNDATA_STRIDE, 0);
        const uint8_t zero = 0;
        const int rc = zkv_sp1_gateway_eth_call_batch(ctx_, n, calldata_blob.empty() ? &zero : calldata_blob.data(), calldata_off.data(), r.reverted.data(),
                                                      r.returndata.data(), r.returndata_len.data(), r.status.data());
        if (rc != ZKV_OK) throw std::runtime_error("zkv_sp1_gateway_eth_call_batch failed with ZKV error " + std::to_string(rc));
        return r;
    }
    // {proofs per route..., not found, shorter than 4 bytes, bad calldata} of the most recent call
    std::vector<uint64_t> last_call_counts() const {
        std::vector<uint64_t> out(route_count() + 3);
        const int rc = zkv_sp1_gateway_last_call_counts(ctx_, out.data());
        if (rc != ZKV_OK) throw std::runtime_error("zkv_sp1_gateway_last_call_counts failed with ZKV error " + std::to_string(rc));
        return out;
    }
    // Opt-in aggregate check on every route (zkv_ctx_set_aggregate_check): sub_batch 0 = automatic size, 16 ... 256 fixed.
    void set_aggregate_check(bool enable, const uint8_t* seed32 = nullptr, int sub_batch = 0) {
        const int rc = zkv_ctx_set_aggregate_check(ctx_, enable ? (sub_batch ? sub_batch : 1) : 0, seed32);
        if (rc != ZKV_OK) throw std::invalid_argument("zkv_ctx_set_aggregate_check failed with ZKV error " + std::to_string(rc));
    }
    zkv_ctx* handle() const { return ctx_; }

private:
    zkv_ctx* ctx_ = nullptr;
};

}  // namespace zkv
