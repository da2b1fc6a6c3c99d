// C++ host wrapper of the RISC Zero verifier router (include/zkv_risc0_router.h): `IRiscZeroVerifier::verify` / `verify_integrity` with
// the verifier chosen per seal by its first 4 bytes, as RISC Zero's on-chain RiscZeroVerifierRouter does.  Library/runtime failures throw
// std::runtime_error; statuses (ZKV_STATUS_*, ZKV_STATUS_ROUTE_NOT_FOUND) are never exceptions.  Parity unpinned: the reference holds no
// router.  RiscZeroSetRouter is the router with a set route (include/zkv_risc0_router_set.h, zkv_risc0_router_set_wire.h).
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/zkv_risc0_router.h"
#include "../../include/zkv_risc0_router_set_wire.h"

namespace zkv {

struct RiscZeroBuiltinRoute {
    std::vector<uint8_t> control_root;       // 32 bytes
    std::vector<uint8_t> bn254_control_id;   // 32 bytes
};

struct RiscZeroKeyedRoute {
    std::vector<uint8_t> vk_words;           // ZKV_RISC0_KEY_BYTES: zkv_groth16_ctx_create's layout with n_ic = 6, RISC Zero's convention
    std::vector<uint8_t> control_root;       // 32 bytes
    std::vector<uint8_t> bn254_control_id;   // 32 bytes
};

class RiscZeroRouter {
public:
    struct Route { uint8_t selector[4]; bool keyed; std::vector<uint8_t> verifier_key_digest; };

    // Route order: the built-in-key routes, then the keyed routes; every selector is derived
    RiscZeroRouter(const std::vector<RiscZeroBuiltinRoute>& builtin, const std::vector<RiscZeroKeyedRoute>& keyed, int device = 0) {
        const Packed p(builtin, keyed);
        ctx_ = zkv_risc0_router_create(builtin.size(), p.roots.data(), p.ids.data(), keyed.size(), p.keys.data(), p.kroots.data(), p.kids.data(), device);
        if (!ctx_) throw std::invalid_argument("zkv_risc0_router_create rejected the routes");
    }
    RiscZeroRouter(RiscZeroRouter&& o) noexcept : ctx_(o.ctx_) { o.ctx_ = nullptr; }
    RiscZeroRouter(const RiscZeroRouter&) = delete;
    RiscZeroRouter& operator=(const RiscZeroRouter&) = delete;
    ~RiscZeroRouter() { if (ctx_) zkv_ctx_destroy(ctx_); }

    size_t route_count() const { return zkv_risc0_router_route_count(ctx_); }
    std::vector<Route> routes() const {
        std::vector<Route> out(route_count());
        for (size_t r = 0; r < out.size(); r++) {
            int keyed = 0;
            out[r].verifier_key_digest.assign(32, 0);
            if (zkv_risc0_router_route(ctx_, r, out[r].selector, &keyed) != ZKV_OK ||
                zkv_risc0_router_route_verifier_key_digest(ctx_, r, out[r].verifier_key_digest.data()) != ZKV_OK) throw std::runtime_error("RiscZeroRouter::routes");
            out[r].keyed = keyed != 0;
        }
        return out;
    }

    // IRiscZeroVerifier as the router forwards it: the status (ZKV_STATUS_OK ... ZKV_STATUS_ROUTE_NOT_FOUND); recv (may be null) gets the received selector
    uint8_t verify(const std::vector<uint8_t>& seal, const uint8_t image_id[32], const uint8_t journal_digest[32], uint8_t recv[4] = nullptr) const {
        uint8_t st = 0;
        const int rc = zkv_risc0_router_verify(ctx_, seal.data(), seal.size(), image_id, journal_digest, &st, recv);
        if (rc != ZKV_OK) throw std::runtime_error("zkv_risc0_router_verify failed with ZKV error " + std::to_string(rc));
        return st;
    }
    uint8_t verify_integrity(const std::vector<uint8_t>& seal, const uint8_t claim_digest[32], uint8_t recv[4] = nullptr) const {
        uint8_t st = 0;
        const int rc = zkv_risc0_router_verify_integrity(ctx_, seal.data(), seal.size(), claim_digest, &st, recv);
        if (rc != ZKV_OK) throw std::runtime_error("zkv_risc0_router_verify_integrity failed with ZKV error " + std::to_string(rc));
        return st;
    }
    // status[i] / recv[4 i .. 4 i + 4) of seal i (ragged host buffers, as zkv_risc0_verify_batch); journal_digests empty: verify_integrity
    // with the claim digests in image_ids
    void verify_batch(const std::vector<uint8_t>& seal_blob, const std::vector<uint64_t>& seal_off, const std::vector<uint8_t>& image_ids,
                      const std::vector<uint8_t>& journal_digests, std::vector<uint8_t>& status, std::vector<uint8_t>& recv) const {
        const size_t n = seal_off.empty() ? 0 : seal_off.size() - 1;
        if (image_ids.size() != 32 * n || (!journal_digests.empty() && journal_digests.size() != 32 * n)) throw std::invalid_argument("RiscZeroRouter::verify_batch: buffer sizes");
        status.assign(n, 0); recv.assign(4 * n, 0);
        const uint8_t zero = 0;
        const uint8_t* blob = seal_blob.empty() ? &zero : seal_blob.data();
        const int rc = journal_digests.empty() && n
            ? zkv_risc0_router_verify_integrity_batch(ctx_, n, blob, seal_off.data(), image_ids.data(), status.data(), recv.data())
            : zkv_risc0_router_verify_batch(ctx_, n, blob, seal_off.data(), image_ids.data(), journal_digests.data(), status.data(), recv.data());
        if (rc != ZKV_OK) throw std::runtime_error("zkv_risc0_router_verify_batch failed with ZKV error " + std::to_string(rc));
    }
    // Device-resident: seals at a stride of ZKV_SEAL_BYTES; d_journal_digests = nullptr: verify_integrity.  Asynchronous on `stream`
    // after one synchronisation with it (the per-route counts).
    void verify_batch_dev(size_t n, const uint8_t* d_seals, const uint8_t* d_image_ids, const uint8_t* d_journal_digests, uint8_t* d_status,
                          uint8_t* d_recv = nullptr, void* stream = nullptr) const {
        const int rc = zkv_risc0_router_verify_batch_dev(ctx_, n, d_seals, d_image_ids, d_journal_digests, d_status, d_recv, stream);
        if (rc != ZKV_OK) throw std::runtime_error("zkv_risc0_router_verify_batch_dev failed with ZKV error " + std::to_string(rc));
    }
    // {seals per route..., selector unknown, shorter than 4 bytes} of the most recent call
    std::vector<uint64_t> last_route_counts() const {
        std::vector<uint64_t> out(route_count() + 2);
        const int rc = zkv_risc0_router_last_route_counts(ctx_, out.data());
        if (rc != ZKV_OK) throw std::runtime_error("zkv_risc0_router_last_route_counts failed with ZKV error " + std::to_string(rc));
        return out;
    }
    // Revert data of a status: SelectorUnknown(bytes4) for ZKV_STATUS_ROUTE_NOT_FOUND, the RISC Zero verifier's bytes otherwise
    std::vector<uint8_t> status_revert(uint8_t status, const uint8_t received[4]) const {
        std::vector<uint8_t> out(68);
        const int n = zkv_risc0_router_status_abi_encode(ctx_, status, received, out.data());
        if (n < 0) throw std::invalid_argument("zkv_risc0_router_status_abi_encode failed with ZKV error " + std::to_string(n));
        out.resize((size_t)n);
        return out;
    }
    // Opt-in aggregate check on the built-in routes and, under the key sets' rules, on the keyed routes (zkv_ctx_set_aggregate_check):
    // sub_batch 0 = automatic size, 16 ... 256 fixed.
    void set_aggregate_check(bool enable, const uint8_t* seed32 = nullptr, int sub_batch = 0) {
        const int rc = zkv_ctx_set_aggregate_check(ctx_, enable ? (sub_batch ? sub_batch : 1) : 0, seed32);
        if (rc != ZKV_OK) throw std::invalid_argument("zkv_ctx_set_aggregate_check failed with ZKV error " + std::to_string(rc));
    }
    zkv_ctx* handle() const { return ctx_; }

protected:
    // the creators' argument rows
    struct Packed {
        std::vector<uint8_t> roots, ids, kroots, kids; std::vector<const uint8_t*> keys;
        Packed(const std::vector<RiscZeroBuiltinRoute>& builtin, const std::vector<RiscZeroKeyedRoute>& keyed) {
            for (const auto& r : builtin) {
                if (r.control_root.size() != 32 || r.bn254_control_id.size() != 32) throw std::invalid_argument("RiscZeroRouter: control parameters must be 32 bytes");
                roots.insert(roots.end(), r.control_root.begin(), r.control_root.end()); ids.insert(ids.end(), r.bn254_control_id.begin(), r.bn254_control_id.end());
            }
            for (const auto& r : keyed) {
                if (r.vk_words.size() != ZKV_RISC0_KEY_BYTES) throw std::invalid_argument("RiscZeroRouter: a keyed route takes a key with n_ic = 6");
                if (r.control_root.size() != 32 || r.bn254_control_id.size() != 32) throw std::invalid_argument("RiscZeroRouter: control parameters must be 32 bytes");
                keys.push_back(r.vk_words.data());
                kroots.insert(kroots.end(), r.control_root.begin(), r.control_root.end()); kids.insert(kids.end(), r.bn254_control_id.begin(), r.bn254_control_id.end());
            }
        }
    };
    explicit RiscZeroRouter(zkv_ctx* adopted) : ctx_(adopted) {}
    zkv_ctx* ctx_ = nullptr;
};

// The router plus the RiscZeroSetVerifier of one set-builder image id, registered under its own selector with the router itself as its
// inner verifier: the last route.  verify / verify_integrity / verify_batch take set-inclusion seals beside Groth16 seals;
// verify_batch_dev (a fixed stride cannot hold a set seal) fails on such a router: use verify_ragged_dev.
class RiscZeroSetRouter : public RiscZeroRouter {
public:
    RiscZeroSetRouter(const uint8_t set_builder_image_id[32], const std::vector<RiscZeroBuiltinRoute>& builtin, const std::vector<RiscZeroKeyedRoute>& keyed,
                      int device = 0) : RiscZeroRouter(create(set_builder_image_id, builtin, keyed, device)) {}

    std::vector<uint8_t> set_selector() const {
        std::vector<uint8_t> out(4);
        const int rc = zkv_risc0_router_set_selector(ctx_, out.data());
        if (rc != ZKV_OK) throw std::runtime_error("zkv_risc0_router_set_selector failed with ZKV error " + std::to_string(rc));
        return out;
    }
    // status of the router's verify(seal, ID, sha256(ID || root)); the root is remembered when that is ZKV_STATUS_OK
    uint8_t submit_root(const uint8_t root[32], const std::vector<uint8_t>& seal, uint8_t recv[4] = nullptr) {
        uint8_t st = 0;
        const int rc = zkv_risc0_router_set_submit_root(ctx_, root, seal.data(), seal.size(), &st, recv);
        if (rc != ZKV_OK) throw std::runtime_error("zkv_risc0_router_set_submit_root failed with ZKV error " + std::to_string(rc));
        return st;
    }
    // Device-resident seals of any length: the blob and its n + 1 offsets; d_journal_digests = nullptr: verify_integrity
    void verify_ragged_dev(size_t n, const uint8_t* d_seal_blob, const uint64_t* d_seal_off, uint64_t blob_bytes, const uint8_t* d_image_ids,
                           const uint8_t* d_journal_digests, uint8_t* d_status, uint8_t* d_recv = nullptr, void* stream = nullptr) const {
        const int rc = zkv_risc0_router_verify_ragged_dev(ctx_, n, d_seal_blob, d_seal_off, blob_bytes, d_image_ids, d_journal_digests, d_status, d_recv, stream);
        if (rc != ZKV_OK) throw std::runtime_error("zkv_risc0_router_verify_ragged_dev failed with ZKV error " + std::to_string(rc));
    }
    // A method per seal (ZKV_METHOD_*; empty: all verify) over ragged host buffers; in_b is not read for verifyIntegrity rows
    void verify_call_batch(const std::vector<uint8_t>& method, const std::vector<uint8_t>& seal_blob, const std::vector<uint64_t>& seal_off,
                           const std::vector<uint8_t>& in_a, const std::vector<uint8_t>& in_b, std::vector<uint8_t>& status, std::vector<uint8_t>& recv) const {
        const size_t n = seal_off.empty() ? 0 : seal_off.size() - 1;
        if (in_a.size() != 32 * n || in_b.size() != 32 * n || (!method.empty() && method.size() != n)) throw std::invalid_argument("RiscZeroSetRouter::verify_call_batch: buffer sizes");
        status.assign(n, 0); recv.assign(4 * n, 0);
        const uint8_t zero = 0;
        const int rc = zkv_risc0_router_verify_call_ragged(ctx_, n, method.empty() ? nullptr : method.data(), seal_blob.empty() ? &zero : seal_blob.data(),
                                                           seal_off.data(), in_a.data(), in_b.data(), status.data(), recv.data());
        if (rc != ZKV_OK) throw std::runtime_error("zkv_risc0_router_verify_call_ragged failed with ZKV error " + std::to_string(rc));
    }
    // eth_call requests in either calldata form, both methods: reverted[i], return / revert data i at returndata[i * ZKV_RETURNDATA_STRIDE ..)
    // with returndata_len[i] bytes, status[i]
    void eth_call_batch(const std::vector<uint8_t>& calldata_blob, const std::vector<uint64_t>& calldata_off, std::vector<uint8_t>& reverted,
                        std::vector<uint8_t>& returndata, std::vector<uint32_t>& returndata_len, std::vector<uint8_t>& status) const {
        const size_t n = calldata_off.empty() ? 0 : calldata_off.size() - 1;
        reverted.assign(n, 0); returndata.assign(n * ZKV_RETURNDATA_STRIDE, 0); returndata_len.assign(n, 0); status.assign(n, 0);
        const uint8_t zero = 0;
        const int rc = zkv_risc0_router_eth_call_ragged(ctx_, n, calldata_blob.empty() ? &zero : calldata_blob.data(), calldata_off.data(), reverted.data(),
                                                        returndata.data(), returndata_len.data(), status.data());
        if (rc != ZKV_OK) throw std::runtime_error("zkv_risc0_router_eth_call_ragged failed with ZKV error " + std::to_string(rc));
    }

private:
    static zkv_ctx* create(const uint8_t set_id[32], const std::vector<RiscZeroBuiltinRoute>& builtin, const std::vector<RiscZeroKeyedRoute>& keyed, int device) {
        const Packed p(builtin, keyed);
        zkv_ctx* c = zkv_risc0_router_create_with_set(builtin.size(), p.roots.data(), p.ids.data(), keyed.size(), p.keys.data(), p.kroots.data(), p.kids.data(),
                                                      set_id, device);
        if (!c) throw std::invalid_argument("zkv_risc0_router_create_with_set rejected the routes");
        return c;
    }
};

}  // namespace zkv
