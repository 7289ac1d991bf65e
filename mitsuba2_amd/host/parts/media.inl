// libmiwave_host: participating media — Medium / HomogeneousMedium, the isotropic and hg phase functions.
// Part of the single translation unit host/miwave_host.cpp (included there, in this order).
// The classes hold what the reference's constructors leave behind and flatten into mi_medium records (include/miwave.h); what
// they evaluate goes through the host compile of the device's leaves (csrc/miw/medium.h).
HGPhaseFunction::HGPhaseFunction(const Properties &props) {
    m_g = props.float_("g", 0.8f);                              // hg.cpp:44-46
    if (m_g >= 1 || m_g <= -1) Throw("The asymmetry parameter must lie in the interval (-1, 1)!");
}
std::shared_ptr<PhaseFunction> make_phase(const Properties &props) {
    if (props.plugin_name() == "isotropic") return std::make_shared<IsotropicPhaseFunction>(props);
    if (props.plugin_name() == "hg") return std::make_shared<HGPhaseFunction>(props);
    Throw("Plugin \"" + props.plugin_name() + "\" not found!");
}
static miw::MediumRec phase_only_record(const PhaseFunction &f) {
    miw::MediumRec r; std::memset(&r, 0, sizeof r);
    r.phase = f.type(); r.g = f.g();
    return r;
}
std::pair<Vector3f, float> PhaseFunction::sample(const Vector3f &ray_d, const std::array<float, 2> &sample) const {
    float pdf = 0.f;
    const miw::V3 wo = miw::phase_sample(phase_only_record(*this), miw::v3(ray_d[0], ray_d[1], ray_d[2]), miw::v2(sample[0], sample[1]), pdf);
    return { Vector3f{ wo.x, wo.y, wo.z }, pdf };
}
float PhaseFunction::eval(const Vector3f &ray_d, const Vector3f &wo) const {
    return miw::phase_eval(phase_only_record(*this), miw::v3(ray_d[0], ray_d[1], ray_d[2]), miw::v3(wo[0], wo[1], wo[2]));
}

Medium::Medium(const Properties &props, std::shared_ptr<PhaseFunction> phase) : m_phase_function(std::move(phase)) {
    if (!m_phase_function) m_phase_function = std::make_shared<IsotropicPhaseFunction>();   // medium.cpp:23-27
    m_sample_emitters = props.bool_("sample_emitters", true);  // :29
}
HomogeneousMedium::HomogeneousMedium(const Properties &props, std::shared_ptr<PhaseFunction> phase) : Medium(props, std::move(phase)) {
    m_is_homogeneous = true;                                   // homogeneous.cpp:22-27
    m_albedo = props.texture("albedo", 0.75f);
    m_sigmat = props.texture("sigma_t", 1.f);
    m_scale = props.float_("scale", 1.0f);
    m_has_spectral_extinction = props.bool_("has_spectral_extinction", true);
}
mi_medium HomogeneousMedium::record() const {
    mi_medium r; std::memset(&r, 0, sizeof r);
    for (int a = 0; a < 3; ++a) { r.sigma_t[a] = m_sigmat[a] * m_scale; r.albedo[a] = m_albedo[a]; }   // eval_sigmat, :30-32
    r.has_spectral_extinction = m_has_spectral_extinction ? 1u : 0u;
    r.sample_emitters = m_sample_emitters ? 1u : 0u;
    r.phase = m_phase_function->type(); r.g = m_phase_function->g();
    return r;
}
static_assert(sizeof(miw::MediumRec) == sizeof(mi_medium), "medium record layout");
