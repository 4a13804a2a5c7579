// antsrl_agent_select_actions.inc — the action part of k_agent_select, ONE text included inside k_agent_select
// (antsrl_memagent.hip) and k_pop_select (antsrl_population.hip); see antsrl_policy_flat_body.inc for why it is an include.
// Reads the including kernel's `a` (SelArgs), `tid` and `nthr` (this thread among the threads that share a's ants).
    for (uint64_t i = tid; i < a.M; i += nthr) {
        const uint32_t e = (uint32_t)i / a.n_ants, ai = (uint32_t)i - e * a.n_ants;
        const bool ex = env_explores(a, e);
        if (ex) {
            const uint64_t env = (uint64_t)a.env_base + e;
            a.rot[i] = (int8_t)((int)draw_below(agent_draw(a.seed, ANTSRL_DRAW_ROTATION, env, a.step, ai), a.n_rot) - (int)(a.n_rot / 2));
            a.ph[i] = (int8_t)draw_below(agent_draw(a.seed, ANTSRL_DRAW_PHEROMONE, env, a.step, ai), a.n_ph);
        }
        if (ai == 0 && a.explored) a.explored[e] = ex ? 1 : 0;
    }
