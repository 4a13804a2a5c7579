// antsrl_agent_select_memory.inc — the memory part of k_agent_select, ONE text included inside k_agent_select
// (antsrl_memagent.hip) and k_pop_memory_select (antsrl_population.hip); see antsrl_policy_flat_body.inc for why it is an
// include.  The ants of an exploring environment get their old memory back (collect_agent_memory.py:204): one thread per
// memory element (V floats), coalesced.  Reads the including kernel's `a` (SelArgs), `tid`, `nthr` and its template
// constant V; it may return, so it stands last in its kernel.
    if (a.mem_old == a.mem_next) return;
    for (uint64_t f = tid; f < a.mem_elems; f += nthr) {
        const uint32_t e = (uint32_t)(f / a.env_elems);
        if (!env_explores(a, e)) continue; // (the draw is cheap next to the forward pass this follows: kept per element)
        if (V == 4)
            reinterpret_cast<float4 *>(a.mem_next)[f] = reinterpret_cast<const float4 *>(a.mem_old)[f];
        else
            a.mem_next[f] = a.mem_old[f];
    }
